"""Per-pixel surface buffers (ft_render_aov, Context.render_aov / pick, functracer --intersection-at): the hit of one sample's geometry
ray of a frame per pixel - t, p, n, colour, material and the leaf / builder node / input triangle it came from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from oracle import ft_oracle_py as O

from . import helpers as H

CHANNELS = ["t", "p", "n", "colour", "material", "leaf", "node", "triangle"]
W, Hh = 160, 90
TILES = [(8, 8, 16, 16), (101, 37, 13, 11), (150, 80, 20, 20)]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_ft_render_aov():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"typedef struct ft_aov\s*\{.*?\}\s*ft_aov;", hdr, flags=re.S)
    assert re.search(r"int32_t ft_render_aov\(ft_context\* ctx, const ft_camera\* cam, int32_t res_h, int32_t res_v, int32_t spp, const double\* jitter_xy,\s*"
                     r"int32_t sample, uint64_t seed, const ft_rect\* tiles, int32_t n_tiles, const ft_aov\* out, ft_stats\* stats\);", hdr)
    assert "#define FT_ABI_VERSION 2" in hdr
    assert hasattr(C.CDLL(ft.HIP_LIB), "ft_render_aov")
    assert C.sizeof(_capi.ft_aov) == 8 * C.sizeof(C.c_void_p)


def _host_only_scene():
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    return ctx


def test_host_only_context_has_no_device():
    ctx = _host_only_scene()
    cam = ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 16 / 9)
    with pytest.raises(_capi.FtError) as e:
        ctx.render_aov(cam, 32, 18, 1, np.zeros((1, 2)))
    assert e.value.status == -2
    ctx.close()


def test_arguments_are_checked_before_anything_runs():
    ctx = _host_only_scene()
    lib, cam = ft.hip_lib(), ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 16 / 9)
    t = np.zeros((18, 32))
    jit = np.zeros((4, 2))
    some, none = _capi.ft_aov(), _capi.ft_aov()
    some.t = _capi.dptr(t)

    def call(spp, sample, aov):
        return lib.ft_render_aov(ctx._ctx, C.byref(cam), 32, 18, spp, _capi.dptr(jit), sample, 1, None, 0, C.byref(aov) if aov is not None else None, None)

    assert call(0, 0, some) == -4                                    # corner sampling: no per-sample geometry ray
    assert call(4, 4, some) == -1 and call(4, -1, some) == -1        # sample outside [0, spp)
    assert call(4, 0, none) == -1 and call(4, 0, None) == -1         # no channel
    assert call(4, 3, some) == -2                                    # valid, but a host-only context renders nothing
    with pytest.raises(ValueError):
        ctx.render_aov(cam, 32, 18, 1, jit[:1], channels=["depth"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _pixel_rays(cam, w, h, pixels, jitter=(0.0, 0.0)):
    o = np.zeros((len(pixels), 3))
    d = np.zeros((len(pixels), 3))
    for k, (x, y) in enumerate(pixels):
        o[k], d[k] = O.ray_through_pixel(cam, w, h, x, y, *jitter)
    return o, d


def _aim(cam, w, h, target):
    """The pixel whose (centre) ray points closest to `target`."""
    o, _ = O.ray_through_pixel(cam, w, h, 0, 0)
    want = np.asarray(target, float) - o
    want /= np.linalg.norm(want)
    best, at = -2.0, None
    for y in range(h):
        for x in range(w):
            _, d = O.ray_through_pixel(cam, w, h, x, y)
            c = float(np.dot(d, want) / np.linalg.norm(d))
            if c > best:
                best, at = c, (x, y)
    return at


def _assert_planes_equal(a, b, names=CHANNELS, what=""):
    for k in names:
        assert np.array_equal(a[k], b[k]), f"{what}: plane {k} differs"


def _bunny_tris():
    with open(os.path.join(H.ROOT, "scenes", "meshes", "bunny_synth_res4.ply")) as f:
        return ft.parse_ply(f.read())


def _oracle_parity(ctx, orc, cam, w, h, tiles, what):
    got = ctx.render_aov(cam, w, h, 1, np.zeros((1, 2)), tiles=tiles)
    if tiles is None:
        pixels = [(x, y) for y in range(h) for x in range(w)]
    else:
        pixels = sorted({(x, y) for (x0, y0, tw, th) in tiles for y in range(max(0, y0), min(h, y0 + th)) for x in range(max(0, x0), min(w, x0 + tw))})
    o, d = _pixel_rays(cam, w, h, pixels)
    whit, wt, wp, wn, wc = orc.closest(o + 1e-4 * d, d)             # slightOffset (Shading.fs:129)
    ys, xs = np.array([p[1] for p in pixels]), np.array([p[0] for p in pixels])
    ghit = (got["leaf"][ys, xs] >= 0).astype(np.int32)
    H.assert_hits_match((ghit, got["t"][ys, xs], got["p"][ys, xs], got["n"][ys, xs], got["colour"][ys, xs]), (whit, wt, wp, wn, wc), what=what)
    m = whit.astype(bool)
    assert np.all(np.isinf(got["t"][ys, xs][~m])) and np.all(got["node"][ys, xs][~m] == -1) and np.all(got["p"][ys, xs][~m] == 0.0)
    assert np.all(got["node"][ys, xs][m] >= 0) and np.all(got["leaf"][ys, xs][m] >= 0)
    assert got["stats"]["rays_primary"] == len(pixels) and got["stats"]["hits_primary"] == int(m.sum())
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. oracle parity
SCENES = sorted(f[:-6] for f in os.listdir(os.path.join(H.ROOT, "scenes")) if f.endswith(".scene"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_aov_matches_the_oracle_on_every_scene(hip, name):
    scene = ft.parse_scene_file(H.scene_path(name))
    cam = scene.camera
    cam.has_focus = 0                                               # pinhole: the oracle's ray_through_pixel is the whole ray
    scene.lower(hip)
    orc = O.Oracle()
    scene.lower(orc)
    _oracle_parity(hip, orc, cam, W, Hh, None, f"{name} full frame")
    _oracle_parity(hip, orc, cam, W, Hh, TILES, f"{name} tiles")


# ---------------------------------------------------------------------------------------------------------------- 2. the render's ray
def _unlit_scene(b):
    """Every object ignoreLight, one light: a sample's colour is exactly its material colour (Shading.fs:100-104), 0 on a miss."""
    b.clear()
    s1 = b.material(b.translate((-1.5, 0, 6), b.primitive(ft.SPHERE)), colour=(0.9, 0.2, 0.1))
    s2 = b.material(b.translate((1.5, 0.3, 9), b.primitive(ft.SPHERE)), colour=(0.1, 0.7, 0.3), roughness=0.4)
    cube = b.material(b.translate((0, -0.5, 4), b.rotate((0, 1, 0), 0.5, b.scale((1.2, 1.2, 1.2), b.primitive(ft.CUBE)))), colour=(0.3, 0.3, 0.9))
    floor = b.texture_grid((1, 1, 1), (0.1, 0.1, 0.1), [(0.0, 0.7, 0.7)], b.translate((0, -1.5, 0), b.primitive(ft.PLANE)))
    b.set_objects(b.group([b.ignore_light(n) for n in (s1, s2, cube, b.hue_shift(1.0, floor))]))
    b.add_directional((0, -1, 1), (1, 1, 1))
    b.commit()


def _focus_camera():
    cam = ft.make_camera((0, 1, -2), (0, 0, 6), (0, 1, 0), H.deg(55), 16 / 9)
    cam.has_focus, cam.focal_length, cam.aperture_angular_size = 1, 7.0, H.deg(3.0)
    return cam


@pytest.mark.gpu
def test_colour_plane_is_the_frame_for_one_sample(hip):
    _unlit_scene(hip)
    cam = _focus_camera()
    jit = ft.jitter_pattern(1)
    frame, _ = hip.render(cam, W, Hh, 1, jit, seed=77)
    got = hip.render_aov(cam, W, Hh, 1, jit, sample=0, seed=77, channels=["colour"])
    assert np.array_equal(got["colour"], frame)
    assert (frame > 0).any() and (frame == 0).all(axis=-1).any()   # hits and misses both present


@pytest.mark.gpu
def test_mean_of_the_sample_planes_is_the_frame_with_depth_of_field(hip):
    _unlit_scene(hip)
    cam = _focus_camera()
    spp = 4
    jit = ft.jitter_pattern(spp)
    frame, _ = hip.render(cam, W, Hh, spp, jit, seed=123)
    acc = np.zeros_like(frame)
    for s in range(spp):
        acc = acc + hip.render_aov(cam, W, Hh, spp, jit, sample=s, seed=123, channels=["colour"])["colour"]
    assert np.array_equal(acc / spp, frame)
    other = hip.render_aov(cam, W, Hh, spp, jit, sample=1, seed=124, channels=["colour"])["colour"]
    assert not np.array_equal(other, hip.render_aov(cam, W, Hh, spp, jit, sample=1, seed=123, channels=["colour"])["colour"])   # the seed keys DoF


# ---------------------------------------------------------------------------------------------------------------- 3. ids
@pytest.mark.gpu
def test_nodes_leaves_and_materials_of_a_hand_built_scene(hip):
    b = hip
    b.clear()
    s1 = b.primitive(ft.SPHERE)
    s2 = b.primitive(ft.SPHERE)
    shared = b.primitive(ft.SPHERE)
    plane = b.primitive(ft.PLANE)
    cube = b.primitive(ft.CUBE)
    carve = b.primitive(ft.SPHERE)
    mats = {"s1": dict(colour=(0.9, 0.1, 0.1), reflectance=0.25, shineyness=12, roughness=0.0),
            "s2": dict(colour=(0.1, 0.9, 0.1), reflectance=0.0, shineyness=3, roughness=0.3),
            "shared": dict(colour=(0.2, 0.2, 0.8), reflectance=0.5, shineyness=0, roughness=0.0),
            "plane": dict(colour=(0.5, 0.5, 0.5), reflectance=0.0, shineyness=0, roughness=0.0),
            "cube": dict(colour=(0.8, 0.6, 0.2), reflectance=0.1, shineyness=20, roughness=0.0),
            "carve": dict(colour=(0.3, 0.9, 0.9), reflectance=0.0, shineyness=5, roughness=0.1)}
    top = [b.material(b.translate((-6, 0, 8), s1), **mats["s1"]),
           b.material(b.translate((6, 0, 8), s2), **mats["s2"]),
           b.material(b.translate((-3, 0, 8), shared), **mats["shared"]),
           b.material(b.translate((3, 0, 8), shared), **mats["shared"]),
           b.material(b.translate((0, -2, 0), plane), **mats["plane"]),
           b.subtract(b.material(b.translate((0, 0, 8), b.scale((2, 2, 2), cube)), **mats["cube"]),
                      b.material(b.translate((0, 0, 7), carve), **mats["carve"]))]
    b.set_objects(b.group(top))
    b.add_directional((0, -1, 1), (1, 1, 1))
    b.commit()
    # (eye above the row of horizontal rays: a ray parallel to a plane below the eye hits it at its origin, Plane.fs:13-16)
    cam = ft.make_camera((0, 0.3, 0), (0, 0.3, 1), (0, 1, 0), H.deg(60), 16 / 9)
    w, h = 192, 108
    got = hip.render_aov(cam, w, h, 1, np.zeros((1, 2)))
    targets = {"s1": ((-6, 0, 8), s1), "s2": ((6, 0, 8), s2), "left": ((-3, 0, 8), shared), "right": ((3, 0, 8), shared),
               "plane": ((9, -2, 40), plane), "cube": ((0.9, 0.9, 7), cube), "carve": ((0, 0, 8), carve)}
    leaves = {}
    for key, (target, node) in targets.items():
        x, y = _aim(cam, w, h, target)
        assert got["node"][y, x] == node, f"{key}: node {got['node'][y, x]}, want {node}"
        assert got["triangle"][y, x] == -1
        leaves[key] = got["leaf"][y, x]
        m = mats["shared" if key in ("left", "right") else key]
        assert np.array_equal(got["colour"][y, x], m["colour"]), key
        assert np.array_equal(got["material"][y, x], [m["reflectance"], m["shineyness"], m["roughness"]]), key
        if key == "carve":                                          # the carved inner wall: B's surface, seen from inside B
            assert got["t"][y, x] > 7.5 and got["n"][y, x][2] < -0.99
    assert leaves["left"] != leaves["right"]                        # one node placed twice: two leaves
    assert len(set(leaves.values())) == len(leaves)
    assert np.unique(got["node"][got["leaf"] >= 0]).tolist() == sorted([s1, s2, shared, plane, cube, carve])


@pytest.mark.gpu
def test_bare_triangles_report_their_own_node(hip):
    b = hip
    b.clear()
    t1 = b.triangle((-2, -1, 5), (-1, 1, 5), (0, -1, 5))
    t2 = b.triangle((0, -1, 5), (1, 1, 5), (2, -1, 5))                # a run of two bare triangles: one leaf, two nodes
    t3 = b.triangle((-1, 0, 6), (0, 1.5, 6), (1, 0, 6))
    b.set_objects(b.group([t1, t2, b.translate((0, 2, 0), t3)]))
    b.commit()
    cam = ft.make_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), H.deg(60), 16 / 9)
    w, h = 96, 54
    got = hip.render_aov(cam, w, h, 1, np.zeros((1, 2)), channels=["node", "triangle", "leaf"])
    leaves = []
    for target, node in (((-1, -0.3, 5), t1), ((1, -0.3, 5), t2), ((0, 2.7, 6), t3)):
        x, y = _aim(cam, w, h, target)
        assert got["node"][y, x] == node and got["triangle"][y, x] == 0
        leaves.append(got["leaf"][y, x])
    assert leaves[0] == leaves[1] != leaves[2]
    assert set(np.unique(got["node"]).tolist()) == {-1, t1, t2, t3}


# ---------------------------------------------------------------------------------------------------------------- 4. triangles
def _bunny_view(b, depth, tris):
    b.clear()
    b.set_objects(b.group([b.material(b.bsp_mesh(depth, tris), colour=(0.8, 0.7, 0.6))]))
    b.add_directional((-1, -1, 1), (1, 1, 1))
    b.commit()
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    c = 0.5 * (lo + hi)
    r = float(np.linalg.norm(hi - lo))
    return ft.make_camera(c + np.array([0.3, 0.4, -1.6]) * r, c, (0, 1, 0), H.deg(40), 16 / 9)


@pytest.mark.gpu
def test_mesh_hits_lie_on_their_input_triangle(hip):
    tris = _bunny_tris()
    cam = _bunny_view(hip, 12, tris)
    got = hip.render_aov(cam, W, Hh, 1, np.zeros((1, 2)))
    m = got["leaf"] >= 0
    assert m.sum() > 500
    k = got["triangle"][m]
    assert k.min() >= 0 and k.max() < tris.shape[0]
    T = tris[k].reshape(-1, 3, 3)
    a, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    v = got["p"][m] - a
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (v * e1).sum(1), (v * e2).sum(1)
    det = g11 * g22 - g12 * g12
    u, w = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    off = v - u[:, None] * e1 - w[:, None] * e2                     # distance from the face's plane
    scale = np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
    assert np.max(np.linalg.norm(off, axis=1) / scale) < 1e-9
    tol = 1e-9
    assert (u >= -tol).all() and (w >= -tol).all() and (u + w <= 1 + tol).all(), "a hit outside the triangle the plane names"
    fn = np.cross(e1, e2)
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    assert np.max(np.linalg.norm(np.cross(got["n"][m], fn), axis=1)) < 1e-6


@pytest.mark.gpu
def test_triangle_plane_is_the_same_for_every_bvh_builder():
    tris = _bunny_tris()
    planes = []
    for builder in (0, 1, 3):
        ctx = ft.Context(device=0)
        ctx.set_option("bvh_builder", builder)
        cam = _bunny_view(ctx, 0, tris)
        planes.append(ctx.render_aov(cam, W, Hh, 1, np.zeros((1, 2)), channels=["triangle", "t", "leaf"]))
        ctx.close()
    assert (planes[0]["triangle"] >= 0).sum() > 500
    for other in planes[1:]:
        _assert_planes_equal(planes[0], other, ["triangle", "t", "leaf"], "bvh_builder")


# ---------------------------------------------------------------------------------------------------------------- 5. invariance
@pytest.mark.gpu
def test_planes_do_not_depend_on_channels_tiles_classification_chunks_or_devices():
    scene = ft.parse_scene_file(H.scene_path("hollow-sphere"))
    cam, w, h = scene.camera, 200, 120
    jit = ft.jitter_pattern(4)
    ctx = ft.Context(device=0)
    scene.lower(ctx)
    full = ctx.render_aov(cam, w, h, 4, jit, sample=2, seed=5)
    assert (full["leaf"] >= 0).sum() > 1000
    for subset in (["t"], ["node", "colour"], ["p", "n", "triangle"], ["material", "leaf"]):
        part = ctx.render_aov(cam, w, h, 4, jit, sample=2, seed=5, channels=subset)
        assert sorted(k for k in part if k != "stats") == sorted(subset)
        _assert_planes_equal(part, full, subset, f"channels {subset}")
    sentinel = {name: np.full((h, w) if wd == 1 else (h, w, wd), 7 if dt == np.int32 else 7.5, dtype=dt) for name, dt, wd, _ in _capi.AOV_CHANNELS}
    tiles = [(0, 0, 64, 32), (70, 40, 37, 23), (190, 100, 40, 40)]
    tiled = ctx.render_aov(cam, w, h, 4, jit, sample=2, seed=5, tiles=tiles, out=sentinel)
    inside = np.zeros((h, w), bool)
    for x0, y0, tw, th in tiles:
        inside[y0:y0 + th, x0:x0 + tw] = True
    for k in CHANNELS:
        assert np.array_equal(tiled[k][inside], full[k][inside]), k
        assert (tiled[k][~inside] == (7 if k in ("leaf", "node", "triangle") else 7.5)).all(), f"{k}: a pixel outside the tiles was written"
    for key, value in (("classify_pixels", 0), ("classify_pixels", 1), ("chunk_samples", 4096)):
        ctx.set_option(key, value)
        _assert_planes_equal(ctx.render_aov(cam, w, h, 4, jit, sample=2, seed=5), full, what=f"{key}={value}")
    ctx.close()
    two = ft.Context(device=[0, 0])
    scene.lower(two)
    got = two.render_aov(cam, w, h, 4, jit, sample=2, seed=5)
    _assert_planes_equal(got, full, what="two devices")
    assert got["stats"]["rays_primary"] == w * h and got["stats"]["hits_primary"] == full["stats"]["hits_primary"]
    two.close()


# ---------------------------------------------------------------------------------------------------------------- 6. no interference
@pytest.mark.gpu
def test_aov_leaves_frames_history_and_queue_as_they_were():
    scene = ft.parse_scene_file(H.scene_path("bunny"))
    cam, w, h = scene.camera, 256, 144
    jit = ft.jitter_pattern(4)
    ref = ft.Context(device=0)
    scene.lower(ref)
    a1, _ = ref.render(cam, w, h, 4, jit)
    a2, _ = ref.render(cam, w, h, 4, jit)                           # a second frame of the same signature (zero-fill / level hint in use)
    ctx = ft.Context(device=0)
    scene.lower(ctx)
    first, _ = ctx.render(cam, w, h, 4, jit)
    assert np.array_equal(first, a1)
    pick = ctx.render_aov(cam, w, h, 4, jit, sample=1, tiles=[(96, 56, 64, 32)])
    assert pick["stats"]["rays_primary"] == 64 * 32
    assert np.array_equal(ctx.fetch_frame(np.zeros((h, w, 3))), a1)   # the frame buffer holds the last render
    second, _ = ctx.render(cam, w, h, 4, jit)
    assert np.array_equal(second, a2)
    # queued frames are retired first, and stay what they were
    ctx.render_enqueue(cam, w, h, 4, jit, seed=1)
    ctx.render_enqueue(cam, w, h, 4, jit, seed=2)
    during = ctx.render_aov(cam, w, h, 4, jit, sample=0)
    ctx.wait()
    _assert_planes_equal(during, ctx.render_aov(cam, w, h, 4, jit, sample=0), what="with frames queued")
    want, _ = ref.render(cam, w, h, 4, jit, seed=2)
    assert np.array_equal(ctx.fetch_frame(np.zeros((h, w, 3))), want)
    ref.close()
    ctx.close()


@pytest.mark.gpu
def test_progressive_accumulation_continues_across_an_aov_call():
    scene = ft.parse_scene_file(H.scene_path("hollow-sphere"))
    cam, w, h = scene.camera, 128, 72
    pieces = [ft.jitter_pattern(2, seed=s) for s in (1, 2, 3)]
    outs = []
    for with_aov in (False, True):
        ctx = ft.Context(device=0)
        scene.lower(ctx)
        ctx.progressive_begin(cam, w, h, tolerance=0.0)
        for k, piece in enumerate(pieces):
            ctx.progressive_pass(2, piece, seed=10 + k)
            if with_aov and k == 0:
                ctx.render_aov(cam, w, h, 2, piece, sample=1, seed=10)
        outs.append(ctx.progressive_fetch())
        ctx.progressive_end()
        ctx.close()
    mean0, _, n0 = outs[0]
    mean1, _, n1 = outs[1]
    assert np.array_equal(mean0, mean1) and np.array_equal(n0, n1)


@pytest.mark.gpu
def test_overflowing_hit_lists_grow_and_the_planes_match_the_oracle():
    tris = _bunny_tris()
    cam = ft.make_camera((0, 1, -6), (0, 0.6, 0), (0, 1, 0), H.deg(40.0), 1.5)

    def build(b):
        b.clear()
        m = b.scale(7.0, b.bsp_mesh(3, tris))
        node = b.subtract(m, b.translate((0.0, 0.9, -0.3), b.scale(0.5, b.primitive(ft.SPHERE))))
        b.set_objects(b.group([b.material(node, colour=(0.8, 0.5, 0.3), reflectance=0.2, shineyness=10)]))
        b.add_directional((-1, -1, 1), (1, 1, 1))
        b.commit()

    ctx = ft.Context(device=0)
    ctx.set_option("csg_mesh_capacity", 2)
    build(ctx)
    small = ctx.scene_info()["csg_capacity"]
    orc = O.Oracle()
    build(orc)
    got = _oracle_parity(ctx, orc, cam, 96, 64, None, "grown hit lists")
    assert ctx.scene_info()["csg_capacity"] > small
    hit = got["leaf"] >= 0
    assert (got["triangle"][hit] >= 0).any() and (got["triangle"][hit] == -1).any()   # bunny faces and the carving sphere's wall
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 7. CLI
@pytest.mark.gpu
def test_cli_intersection_at_prints_the_pick_record(hip):
    path = H.scene_path("bunny")
    scene = ft.parse_scene_file(path)
    res_h, res_v = scene.resolution
    scene.lower(hip)
    cli = os.path.join(H.ROOT, "functracer_amd", "lib", "functracer")
    leaf = hip.render_aov(scene.camera, res_h, res_v, 1, np.zeros((1, 2)), channels=["leaf"])["leaf"]
    ys, xs = np.nonzero(leaf >= 0)
    hx, hy = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])           # a pixel that sees the bunny
    for x, y in ((hx, hy), (3, 2)):
        out = subprocess.run([cli, path, "--intersection-at", str(x), str(y)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout == ""                                     # no image
        want = hip.pick(scene.camera, res_h, res_v, x, y)
        rec = dict(re.findall(r"^(\w+) = (.*)$", out.stderr, flags=re.M))
        if want is None:
            assert "None" in out.stderr and not rec
            continue
        for k, v in want.items():
            vals = [float(s) for s in rec[k].split()] if isinstance(v, tuple) else ([int(rec[k])] if isinstance(v, int) else [float(rec[k])])
            assert vals == (list(v) if isinstance(v, tuple) else [v]), k
    assert hip.pick(scene.camera, res_h, res_v, hx, hy)["triangle"] >= 0

"""Light-space shadow trees (ft_flat.h, kLsPairDoubles): the host builder's boxes hold every triangle they lead to, degenerate
directions and the pair cap give "none", and on the device the walk changes no bit of any frame or counter."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import functracer_amd as ft
from tests.helpers import ROOT, scene_path

PAIR_DOUBLES, NODE_WORDS, MAX_PAIRS = 16, 24, 64
NONE = -(1 << 31)


def light_space(ctx):
    lib = ctx._lib
    lib.ft_debug_light_space.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    sizes = (C.c_int64 * 4)()
    ctx._check(lib.ft_debug_light_space(ctx._ctx, sizes, None, None, None, None))
    pairs = np.zeros((sizes[0], PAIR_DOUBLES))
    nodes = np.zeros((sizes[1], NODE_WORDS), dtype=np.uint32)
    tris = np.zeros((sizes[2], 9))
    leaf_pairs = np.zeros(sizes[3], dtype=np.uint32)
    ctx._check(lib.ft_debug_light_space(ctx._ctx, sizes, pairs.ctypes.data, nodes.ctypes.data, tris.ctypes.data, leaf_pairs.ctypes.data))
    return pairs, nodes, tris, leaf_pairs


def pair_root(rec):
    return int(rec[14:15].view(np.int32)[0])


def bunny_tris():
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_res4.ply")) as f:
        return ft.parse_ply(f.read())


def mesh_scene(b, tris, lights, xf=None, copies=1):
    b.clear()
    items = []
    for k in range(copies):
        node = b.bsp_mesh(0, tris)
        node = b.transform(xf + [("translate", (3.0 * k, 0, 0))] if xf else [("translate", (3.0 * k, 0, 0))], node)
        items.append(b.material(node, colour=(0.8, 0.7, 0.6)))
    b.set_objects(b.group(items))
    for kind, v in lights:
        if kind == "dir":
            b.add_directional(v, (1, 1, 1))
        else:
            b.add_positional(v, (1, 0.01, 0.02), (1, 1, 1))
    b.commit()


def check_tree(rec, nodes, ls_tris):
    """Every triangle record a leaf holds, projected into the pair's frame and widened by the box inflation the builder promises
    against rounding (none here: the exact footprint), lies inside the (u, v) rectangle and under the w bound of every node on its path."""
    U, V, D, c = rec[0:3], rec[3:6], rec[6:9], rec[9:12]
    seen = 0
    stack = [(pair_root(rec), [])]
    while stack:
        n, path = stack.pop()
        boxes = nodes[n, :20].view(np.float32).reshape(4, 5)
        kids = nodes[n, 20:24].view(np.int32)
        for k in range(4):
            ch = int(kids[k])
            if ch == NONE:
                assert np.isnan(boxes[k]).all()
                continue
            p = path + [boxes[k]]
            if ch >= 0:
                stack.append((ch, p))
                continue
            first, count = (~ch) >> 3, (~ch) & 7
            assert 1 <= count <= 7
            for t in ls_tris[first:first + count]:
                v0 = t[0:3] - c
                for q in (v0, v0 + t[3:6], v0 + t[6:9]):
                    u, v, w = q @ U, q @ V, q @ D
                    for bx in p:
                        assert bx[0] <= u <= bx[1] and bx[2] <= v <= bx[3] and w <= bx[4]
                seen += 1
    return seen


def test_boxes_hold_their_triangles_and_leaves_copy_the_records():
    tris = bunny_tris()
    ctx = ft.Context(host_only=True)
    xf = [("scale", (8.0, 3.0, 5.0)), ("rotate", (1.0, 2.0, 3.0), 0.7)]
    mesh_scene(ctx, tris, [("dir", (-3, -2, 3)), ("point", (0, 5, 0)), ("dir", (0, -1, 0))], xf=xf)
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    assert leaf_pairs[0] != 0xFFFFFFFF
    recs = pairs[leaf_pairs[0]:leaf_pairs[0] + 3]
    assert pair_root(recs[1]) == NONE                                  # a point light has no tree
    want = {tuple(np.concatenate([t[0:3], t[3:6] - t[0:3], t[6:9] - t[0:3]]).tolist()) for t in tris}
    for l in (0, 2):
        rec = recs[l]
        assert pair_root(rec) >= 0
        U, V, D = rec[0:3], rec[3:6], rec[6:9]
        frame = np.array([U, V, D])
        assert np.allclose(frame @ frame.T, np.eye(3), atol=1e-14)
        assert check_tree(rec, nodes, ls_tris) == len(tris)
    assert {tuple(r.tolist()) for r in ls_tris} == want                # bitwise copies of the mesh's own records
    ctx.close()


def test_axis_aligned_light_gets_an_orthonormal_frame():
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, bunny_tris(), [("dir", (0, 0, 1)), ("dir", (1, 0, 0))])
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    for l in range(2):
        rec = pairs[leaf_pairs[0] + l]
        frame = np.array([rec[0:3], rec[3:6], rec[6:9]])
        assert np.isfinite(frame).all() and np.allclose(frame @ frame.T, np.eye(3), atol=1e-15)
        assert check_tree(rec, nodes, ls_tris) == 980
    ctx.close()


def test_degenerate_direction_gets_none():
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, bunny_tris(), [("dir", (0, 0, 0)), ("dir", (1, -1, 0))])
    pairs, _, _, leaf_pairs = light_space(ctx)
    assert pair_root(pairs[leaf_pairs[0]]) == NONE and pair_root(pairs[leaf_pairs[0] + 1]) >= 0
    ctx.close()


def test_pair_cap_holds():
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, bunny_tris()[:64], [("dir", (-3, -2, 3))], copies=MAX_PAIRS + 6)
    pairs, _, _, leaf_pairs = light_space(ctx)
    with_tree = sum(1 for k in leaf_pairs if k != 0xFFFFFFFF and pair_root(pairs[k]) >= 0)
    assert with_tree == MAX_PAIRS
    ctx.close()


def test_option_off_builds_nothing():
    ctx = ft.Context(host_only=True)
    ctx.set_option("light_space_shadows", 0)
    mesh_scene(ctx, bunny_tris(), [("dir", (-3, -2, 3))])
    _, _, _, leaf_pairs = light_space(ctx)
    assert (leaf_pairs == 0xFFFFFFFF).all()
    ctx.close()


# ---- on the device: the walk changes no bit ----------------------------------------------------------------------------------------

def render_both(ctx, lower, cam, w, h, spp):
    jit = ft.jitter_pattern(spp)
    out = []
    for opt in (0, 1):
        ctx.set_option("light_space_shadows", opt)
        lower(ctx)
        img, st = ctx.render(cam, w, h, spp, jit)
        out.append((img, {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}))
    (a, sa), (b, sb) = out
    assert np.array_equal(a, b), f"frames differ on {np.count_nonzero(np.any(a != b, axis=2))} pixels"
    assert sa == sb
    return a, sa


def camera_at(o, look):
    return ft.make_camera(o, look, (0, 1, 0), math.radians(60), 1.0)


def built(tris, lights, xf=None, extra=None):
    def lower(ctx):
        ctx.clear()
        node = ctx.bsp_mesh(0, tris)
        if xf:
            node = ctx.transform(xf, node)
        items = [ctx.material(node, colour=(0.8, 0.7, 0.6))]
        if extra:
            items += extra(ctx)
        ctx.set_objects(ctx.group(items))
        for kind, v in lights:
            if kind == "dir":
                ctx.add_directional(v, (1, 1, 1))
            else:
                ctx.add_positional(v, (1, 0.01, 0.02), (1, 1, 1))
        ctx.commit()
    return lower


@pytest.mark.gpu
def test_headline_scene_identical(hip):
    p = ft.parse_scene_file(scene_path("bunny"))
    _, st = render_both(hip, p.lower, p.camera, 480, 270, 4)
    assert st["rays_shadow"] > 0


@pytest.mark.gpu
def test_scaled_rotated_bunny_identical(hip):
    xf = [("scale", (8.0, 3.0, 5.0)), ("rotate", (1.0, 2.0, 3.0), 0.7)]
    render_both(hip, built(bunny_tris(), [("dir", (-3, -2, 3))], xf=xf), camera_at((0, 2, -4), (0, 0, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_axis_light_identical(hip):
    xf = [("scale", (8.0, 8.0, 8.0))]
    render_both(hip, built(bunny_tris(), [("dir", (0, -1, 0))], xf=xf), camera_at((0, 2, -3), (0, 0.5, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_grazing_light_on_flat_mesh_identical(hip):
    g = np.linspace(-1.0, 1.0, 9)
    quads = []
    for i in range(8):
        for j in range(8):
            a, b, c, d = (g[i], 0, g[j]), (g[i + 1], 0, g[j]), (g[i + 1], 0, g[j + 1]), (g[i], 0, g[j + 1])
            quads += [[*a, *b, *c], [*a, *c, *d]]
    tris = np.array(quads, dtype=np.float64)
    bunny = lambda ctx: [ctx.material(ctx.transform([("scale", (4.0, 4.0, 4.0))], ctx.bsp_mesh(0, bunny_tris())), colour=(1, 1, 1))]
    render_both(hip, built(tris, [("dir", (1, 0, 0)), ("dir", (0, 0, -1))], xf=[("scale", (3.0, 3.0, 3.0))], extra=bunny),
                camera_at((0, 3, -5), (0, 0, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_two_directional_and_a_point_light_identical(hip):
    xf = [("scale", (8.0, 8.0, 8.0)), ("rotate", (0.0, 1.0, 0.0), math.pi)]
    render_both(hip, built(bunny_tris(), [("dir", (-3, -2, 3)), ("point", (1, 4, -2)), ("dir", (2, -1, 1))], xf=xf),
                camera_at((0, 2, -2), (0, 0, 3)), 256, 256, 2)


@pytest.mark.gpu
def test_mesh_beside_csg_identical(hip):
    def csg(ctx):
        a = ctx.translate((1.5, 0.5, 0.0), ctx.primitive(ft.SPHERE))
        b = ctx.translate((1.9, 0.5, 0.0), ctx.primitive(ft.CUBE))
        return [ctx.material(ctx.subtract(a, b), colour=(0.3, 0.6, 0.9)), ctx.material(ctx.primitive(ft.PLANE), colour=(0.5, 0.5, 0.5))]
    render_both(hip, built(bunny_tris(), [("dir", (-3, -2, 3))], xf=[("scale", (8.0, 8.0, 8.0))], extra=csg),
                camera_at((0, 2, -4), (0.5, 0.5, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_large_mesh_device_built_identical(hip):
    path = os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")
    with open(path) as f:
        tris = ft.parse_ply(f.read())
    assert len(tris) >= 4096
    render_both(hip, built(tris, [("dir", (-3, -2, 3))], xf=[("scale", (8.0, 8.0, 8.0))]), camera_at((0, 2, -2), (0, 0.5, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_recommit_after_light_change_identical(hip):
    xf = [("scale", (8.0, 8.0, 8.0))]
    cam = camera_at((0, 2, -2), (0, 0.5, 0))
    a, _ = render_both(hip, built(bunny_tris(), [("dir", (-3, -2, 3))], xf=xf), cam, 192, 192, 2)
    b, _ = render_both(hip, built(bunny_tris(), [("dir", (3, -2, -1))], xf=xf), cam, 192, 192, 2)
    assert not np.array_equal(a, b)                                    # the shadows moved


@pytest.mark.gpu
def test_two_device_context_on_one_gpu_identical():
    ctx = ft.Context(device=[0, 0])
    try:
        p = ft.parse_scene_file(scene_path("bunny"))
        render_both(ctx, p.lower, p.camera, 320, 180, 2)
    finally:
        ctx.close()

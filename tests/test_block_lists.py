"""Per-block triangle candidate lists (k_block_lists; option primary_block_lists): the primaries of a block that carries a list test
its entries instead of walking the mesh's tree.  A list holds every triangle a ray of the block can hit, and the closest hit does not
depend on the order triangles are offered in (ties go by list index), so no bit of any frame or counter may move with the option."""
import math

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from tests.test_light_space_shadows import built, bunny_tris, camera_at

LIGHTS = [("dir", (-3, -2, 3)), ("point", (1, 4, -2))]


def wavy(n, half=1.0, amp=0.15):
    """A height field over [-half, half]^2 in the xz plane, 2 n^2 triangles."""
    g = np.linspace(-half, half, n + 1)
    hgt = lambda x, z: amp * math.sin(3.0 * x) * math.cos(2.0 * z)
    quads = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = [(x, hgt(x, z), z) for x, z in ((g[i], g[j]), (g[i + 1], g[j]), (g[i + 1], g[j + 1]), (g[i], g[j + 1]))]
            quads += [[*a, *c, *b], [*a, *d, *c]]                              # wound so that the normals point up, at the cameras and the lights
    return np.array(quads, dtype=np.float64)


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}


def render_both(ctx, lower, cam, w, h, spp, **kw):
    """The frame with the lists off and on: equal bit for bit, every counter too.  Returns the frame, the counters and the lists."""
    jit = ft.jitter_pattern(spp)
    lower(ctx)
    out = []
    try:
        for opt in (0, 1):
            ctx.set_option("primary_block_lists", opt)
            img, st = ctx.render(cam, w, h, spp, jit, **kw)
            out.append((img, counters(st)))
        lists = ctx.block_lists()
    finally:
        ctx.set_option("primary_block_lists", 1)
    (a, sa), (b, sb) = out
    assert np.array_equal(a, b), f"frames differ on {np.count_nonzero(np.any(a != b, axis=2))} pixels"
    assert sa == sb
    return a, sa, lists


def listed(lists):
    return lists["heads"] != _capi.LIST_NONE


def some_listed(lists):
    """The frame carried lists and at least one active block tests a non-empty one: the case does not pass on the walk alone."""
    assert lists["leaf"] >= 0 and listed(lists).any() and lists["entries"].size > 0, (lists["leaf"], int(listed(lists).sum()), lists["entries"].size)


def faces_per_block(ctx, lists):
    """The source faces in each listed block's list, by position among the active blocks."""
    face = ctx.mesh_trees()["tri_src"][lists["entries"]["orig"]]
    return {pos: set(int(f) for f in face[head >> 7:(head >> 7) + (head & 127)]) for pos, head in enumerate(int(h) for h in lists["heads"]) if head != _capi.LIST_NONE}


def with_filler(tris):
    """Meshes under eight triangles get no tree, so no lists: eight small triangles far outside every view of these tests, after the
    mesh's own (whose face numbers stay)."""
    far = [[1000.0 + 3 * k, 1000.0, 1000.0, 1001.0 + 3 * k, 1000.0, 1000.0, 1000.0 + 3 * k, 1001.0, 1000.0] for k in range(8)]
    return np.array(list(tris) + far, dtype=np.float64)


MAIN_MESH = dict(tris=wavy(6), xf=[("scale", (3.0, 3.0, 3.0))])
MAIN_CAM = ((0.2, 2.5, -3.0), (0, 0, 0))


def main_scene():
    return built(MAIN_MESH["tris"], LIGHTS, xf=MAIN_MESH["xf"])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", [(64, 48, 16), (128, 96, 4)])
def test_main_case_blocking_queued_and_superset(hip, w, h, spp):
    cam = camera_at(*MAIN_CAM)
    jit = ft.jitter_pattern(spp)
    frame, st, L = render_both(hip, main_scene(), cam, w, h, spp)
    assert st["hits_primary"] > 0 and frame.max() > 0.05                   # lit, so that a wrong hit shows in the frame
    # the test must not pass on fallbacks alone
    n_active, n_listed = len(L["heads"]), int(listed(L).sum())
    assert L["leaf"] >= 0 and n_active > 0 and 2 * n_listed >= n_active, (n_active, n_listed)
    assert L["entries"]["x0"].size > 0 and int((L["heads"][listed(L)] & 127).max()) <= 64
    # superset: the triangle every sample hits is in its block's list, the sample's point on the image plane inside its rectangle
    tri_src = hip.mesh_trees()["tri_src"]
    tlx, tly, pw, ph = L["plane"]
    pos_of = {int(b): k for k, b in enumerate(L["pos_block"])}
    ent = L["entries"]
    face = tri_src[ent["orig"]]
    checked = 0
    for s in range(spp):
        tri = hip.render_aov(cam, w, h, spp, jit, sample=s, channels=["triangle"])["triangle"]
        for y, x in zip(*np.nonzero(tri >= 0)):
            pos = pos_of.get((int(y) // 8) * (w // 8) + int(x) // 8)
            assert pos is not None, f"pixel ({x}, {y}) is hit but its block is not active"
            head = int(L["heads"][pos])
            if head == _capi.LIST_NONE:
                continue
            e, f = ent[head >> 7:(head >> 7) + (head & 127)], face[head >> 7:(head >> 7) + (head & 127)]
            jx, jy = tlx + (x + jit[s, 0]) * pw, tly - (y - jit[s, 1]) * ph
            ok = (f == tri[y, x]) & (e["x0"] <= jx) & (jx <= e["x1"]) & (e["y0"] <= jy) & (jy <= e["y1"])
            assert ok.any(), f"sample {s} of pixel ({x}, {y}) hits face {tri[y, x]}: not in its block's list"
            checked += 1
    assert checked > 0
    # three frames queued: each equals the blocking frame, with the lists and without
    with ft.PinnedArray((3, h, w, 3)) as pinned:
        queued = {}
        try:
            for opt in (1, 0):
                hip.set_option("primary_block_lists", opt)
                pinned[:] = -1.0
                for k in range(3):
                    hip.render_enqueue(cam, w, h, spp, jit, out=pinned[k])
                queued[opt] = counters(hip.wait())
                for k in range(3):
                    assert np.array_equal(pinned[k], frame), (opt, k)
            assert queued[0] == queued[1]
            assert all(queued[1][k] == st[k] for k in st if k.startswith(("rays_", "hits_", "csg_")))
        finally:
            hip.set_option("primary_block_lists", 1)


@pytest.mark.gpu
def test_dense_mesh_overflows_into_the_walk(hip):
    _, _, L = render_both(hip, built(wavy(40), LIGHTS, xf=[("scale", (3.0, 3.0, 3.0))]), camera_at(*MAIN_CAM), 32, 24, 4)
    assert L["leaf"] >= 0 and (~listed(L)).any()                              # 3200 triangles under at most 12 blocks: some hold over 64


@pytest.mark.gpu
def test_triangles_across_the_camera_plane_and_camera_inside_the_box(hip):
    """The camera hovers inside the mesh's bounding box, just above the surface: triangles beside and behind it cross its plane."""
    lower = built(wavy(6), LIGHTS, xf=[("scale", (3.0, 3.0, 3.0))])
    for cam in (camera_at((0.1, 0.2, -0.4), (0.3, 0.0, 2.0)), camera_at((0.0, 0.05, 0.0), (1.0, 0.3, 1.0))):
        _, st, L = render_both(hip, lower, cam, 64, 48, 4)
        some_listed(L)
        assert st["hits_primary"] > 0 and np.isinf(L["entries"]["x0"]).any()  # a triangle at the camera plane: an unbounded rectangle


@pytest.mark.gpu
def test_one_triangle_covers_the_frame(hip):
    big = [[-50, -50, 5, 50, -50, 5, 0, 80, 5], [-0.5, -0.5, 3, 0.5, -0.5, 3, 0, 0.5, 3]]
    _, st, L = render_both(hip, built(with_filler(big), LIGHTS), camera_at((0, 0, -2), (0, 0, 1)), 64, 48, 4)
    assert st["hits_primary"] == 64 * 48 * 4
    # every block of the frame is active and tests a list, the covering triangle is in each, the small one in some and not in all
    per_block = faces_per_block(hip, L)
    assert L["leaf"] >= 0 and len(L["heads"]) == 48 and len(per_block) == 48
    assert all(0 in f for f in per_block.values())
    assert 0 < sum(1 in f for f in per_block.values()) < 48


@pytest.mark.gpu
def test_edge_on_pair_ties_by_list_index(hip):
    """Two triangles that share an edge, both in the plane y = 0 the camera lies in, and a third one folded up from the shared edge."""
    tris = [[-1, 0, 2, 1, 0, 2, 0, 0, 4], [1, 0, 2, -1, 0, 2, 0, 0, 1], [-1, 0, 2, 1, 0, 2, 0, 1.5, 2.5]]
    lower = built(with_filler(tris), LIGHTS)
    for cam in (camera_at((0, 0, -2), (0, 0, 1)), camera_at((0, 1e-9, -2), (0, 0, 1))):
        _, st, L = render_both(hip, lower, cam, 64, 48, 4)
        some_listed(L)
        # the pair and the fold meet in one block's list, so that the rays along the shared edge choose among them there
        assert st["hits_primary"] > 0 and any({0, 1, 2} <= f for f in faces_per_block(hip, L).values())


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["far", "small", "large"])
def test_camera_far_from_the_origin_and_scene_scales(hip, where):
    s, off = {"far": (3.0, 1e6), "small": (3e-3, 0.0), "large": (3e3, 0.0)}[where]
    xf = [("scale", (s, s, s)), ("translate", (off, off, off))]
    k = s / 3.0
    cam = camera_at((off + 0.2 * k, off + 2.5 * k, off - 3.0 * k), (off, off, off))
    _, st, L = render_both(hip, built(wavy(6), LIGHTS, xf=xf), cam, 64, 48, 4)
    some_listed(L)
    assert st["hits_primary"] > 0 and 2 * int(listed(L).sum()) >= len(L["heads"])   # the main case's mesh and view: as many lists as there


@pytest.mark.gpu
def test_paths_that_stay_on_the_walk(hip):
    cam = camera_at(*MAIN_CAM)
    lower = main_scene()
    render_both(hip, lower, cam, 64, 48, 3)                                  # plain numbering
    render_both(hip, lower, cam, 60, 44, 4)                                  # the pixel list is not made of whole blocks
    render_both(hip, lower, cam, 64, 48, 4, tiles=[(0, 8, 64, 8), (0, 24, 64, 16)])   # bands
    dof = camera_at(*MAIN_CAM)
    dof.has_focus, dof.focal_length, dof.aperture_angular_size = 1, 3.5, math.radians(2.0)
    render_both(hip, lower, dof, 64, 48, 4)
    # a sphere that touches the mesh: hits at equal distance go to the earlier item, whichever way the mesh was searched
    sphere = lambda ctx: [ctx.material(ctx.transform([("translate", (0.0, 0.9, 0.0))], ctx.primitive(ft.SPHERE)), colour=(0.2, 0.4, 0.9))]
    render_both(hip, built(MAIN_MESH["tris"], LIGHTS, xf=MAIN_MESH["xf"], extra=sphere), cam, 64, 48, 4)


@pytest.mark.gpu
def test_camera_changes_between_queued_frames(hip):
    """Every queued frame's list is its own: three cameras in flight give the three blocking frames."""
    w, h, spp = 64, 48, 4
    jit = ft.jitter_pattern(spp)
    cams = [camera_at((0.2, 2.5, -3.0), (0, 0, 0)), camera_at((2.0, 1.5, -2.0), (0.5, 0, 0)), camera_at((-1.0, 3.0, 1.0), (0, 0, -0.5))]
    main_scene()(hip)
    try:
        hip.set_option("primary_block_lists", 0)
        want = [hip.render(c, w, h, spp, jit)[0] for c in cams]
        hip.set_option("primary_block_lists", 1)
        with ft.PinnedArray((6, h, w, 3)) as pinned:
            pinned[:] = -1.0
            for k in range(6):
                hip.render_enqueue(cams[k % 3], w, h, spp, jit, out=pinned[k])
            hip.wait()
            for k in range(6):
                assert np.array_equal(pinned[k], want[k % 3]), k
    finally:
        hip.set_option("primary_block_lists", 1)
    assert not np.array_equal(want[0], want[1])

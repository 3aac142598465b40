"""k_primary_mesh (option primary_mesh_kernel): bounce 0 of a scene that is one lit bare mesh under directional lights runs a kernel
of its own, built from k_primary's device functions without the code such a scene never reaches.  Every value that reaches a pixel or
a counter comes from the same expression either way, so with the option 0 and 1 every frame and every ft_stats counter is equal bit
for bit; each frame is also held against the CPU oracle.  Context.primary_kernels() says which kernel the bounce-0 launches went to:
the qualifying cases must take the new one, and every scene, camera, option or call the kernel is not written for must not.

The CPU half proves on the oracle that each case shows what it is there for: hits on at least a tenth of the frame, at least 32 of them
in the mesh's own shadow where the mesh can cast one, lit ones and misses beside them; and on a host-only context that the meshes have
the light-space structures the cases name.  The views were found by a search on the oracle alone: a seen triangle, an occluder among
its neighbours, the light along the line from the occluder to the seen one, the eye on the lit side."""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from oracle import ft_oracle_py as O

from . import bvh_tools as B
from . import helpers as H
from . import shadow_tools as S
from . import walk_tools as W
from .test_light_space_grid import grid_of

gpu = pytest.mark.gpu
WID, HGT = 72, 56                                                   # 9 x 7 blocks of 8 x 8: the frames are classified and carry candidate lists
GENERAL, HAIR = S.GENERAL, S.HAIR                                   # HAIR: a hair off the y axis (1e-4, -1, 3e-5)

# mesh: a catalogue entry; ops: its transform; lights: directions; spp: 2 - a wave is 32 pixels under 2 offsets, 4 - 4x4 squares under 4,
# 16 - 2x2 squares under 16, 32 - the same, two offset groups per block (s0 != 0); material: keywords of b.material; shadows: the mesh
# shades itself under lights[0] in this view; qualifies: the frame takes k_primary_mesh
Case = namedtuple("Case", "mesh ops lights eye look fov spp material shadows qualifies", defaults=(True,))
_M = dict(colour=(0.8, 0.7, 0.6))
CASES = {
    "blob(8)": Case("blob(8)", None, [(-0.6604, 0.6128, -0.434)], (0.0818, 0.5731, -0.7186), (-0.0416, 0.4698, -0.7161), 30.0, 4, _M, True),
    "blob(65)": Case("blob(65)", None, [(0.6358, -0.5702, 0.5202), GENERAL, HAIR], (-1.1377, -1.2663, 0.0162), (-0.9479, -1.147, 0.0176), 30.0, 16,
                     dict(colour=(0.8, 0.7, 0.6), shineyness=4.0), True),             # three lights, an integral specular exponent
    "blob(65)-xf": Case("blob(65)", list(W.XF), [(0.0074, 0.676, 0.7369)], (0.4192, 0.9693, 0.6021), (0.5135, 0.9119, 0.6484), 30.0, 4, _M, True),
    "blob(65)-mirror": Case("blob(65)", list(W.XF) + S.MIRROR, [(-0.1731, 0.9849, -0.0034), HAIR], (-0.2729, -0.5383, 0.2644), (-0.3697, -0.3239, 0.4495), 30.0, 2,
                            dict(colour=(0.8, 0.7, 0.6), shineyness=3.0), True),
    "spanning": Case("spanning", None, [(-0.6009, -0.162, -0.7828)], (-0.1356, -0.5782, 0.3244), (-0.0364, -0.7113, 0.1828), 30.0, 32, _M, True),
    "degenerate": Case("degenerate", None, [(-0.2074, 0.9561, -0.2069), GENERAL, HAIR], (0.2027, -0.3924, -0.2423), (0.1238, -0.2788, -0.3352), 45.0, 16, _M, True),
    "concentric": Case("concentric", None, [(-0.5774, -0.5774, -0.5774)], (1.272, 1.0065, 0.1235), (-0.2123, -0.2123, -0.2123), 30.0, 4, _M, True),
    # 300 times one triangle: nothing of it stands between another part of it and any light (walk_tools.NO_SELF_SHADOW)
    "identical": Case("identical", None, [GENERAL], None, None, None, 16, _M, False),
    "two_clusters": Case("two_clusters", None, [(0.814, 0.1339, -0.5652)], (-0.002, -0.0043, -0.0046), (-0.0011, 0.0007, -0.0041), 30.0, 4, _M, True),
    # A mesh of fewer than 8 triangles gets neither pairs nor a BVH (ft_scene.cpp, bvh_for_leaf): k_primary tests its triangles one by one,
    # and the kernel written for a mesh WITH a tree must leave it alone.  (A leaf with a tree and without pairs - mesh_bvh_packet<true>
    # answering the shadow rays - is what light_space_shadows = 0 makes of blob(65) in the options test.)
    "blob(7)": Case("blob(7)", None, [(0.6069, 0.0618, 0.7923)], (0.3329, -0.1416, 0.4127), (0.441, -0.1161, 0.5898), 45.0, 16, _M, True, False),
}
NAMES = list(CASES)


def tris_of(case):
    return B.catalogue()[case.mesh].tris


def camera_of(case):
    if case.eye is None:                                            # walk_tools' outside view of the mesh
        v = W.shallow_views(case.mesh)[0]
        return ft.make_camera(tuple(v.o), tuple(v.look), (0, 1, 0), math.radians(v.fov), WID / HGT)
    return ft.make_camera(case.eye, case.look, (0, 1, 0), math.radians(case.fov), WID / HGT)


def lower_mesh(tris, ops=None, lights=(GENERAL,), material=_M, depth=0, unlit=False, extra=None, point=None):
    """lower(builder): one `bspMesh depth` of `tris` under `ops` and directional `lights`; extra(b): more top-level items."""
    def lower(b):
        b.clear()
        node = b.bsp_mesh(depth, np.asarray(tris).reshape(-1, 9))
        if ops:
            node = b.transform(list(ops), node)
        item = b.material(node, **material)
        if unlit:
            item = b.ignore_light(item)
        b.set_objects(b.group([item] + (extra(b) if extra else [])))
        for v in lights:
            b.add_directional(tuple(v), (1, 1, 1))
        if point is not None:
            b.add_positional(tuple(point), (1.0, 0.0, 0.02), (0.5, 0.5, 1.0))
        b.commit()
    return lower


def lower_of(case):
    return lower_mesh(tris_of(case), case.ops, case.lights, case.material)


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """The oracle's frame of a case, rendered once and shared."""
    case = CASES[name]
    orc = O.Oracle()
    lower_of(case)(orc)
    frame, _ = orc.render(camera_of(case), WID, HGT, case.spp, ft.jitter_pattern(case.spp))
    orc.close()
    frame.setflags(write=False)
    return frame


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}


# =============================================================================================================================
# CPU half

@pytest.mark.parametrize("name", NAMES)
def test_case_shows_hits_shadows_and_misses_on_the_oracle(name):
    case = CASES[name]
    cam = camera_of(case)
    o, d = np.zeros((WID * HGT, 3)), np.zeros((WID * HGT, 3))
    for k in range(WID * HGT):
        o[k], d[k] = O.ray_through_pixel(cam, WID, HGT, k % WID, k // WID, 0.0, 0.0)
    orc = O.Oracle()
    lower_of(case)(orc)
    hit, _, p, n, _ = orc.closest(o + W.SLIGHT_OFFSET * d, d)
    m = hit.astype(bool)
    shadowed = [orc.blocked(p[m] + W.SLIGHT_OFFSET * n[m], np.broadcast_to(-np.asarray(v, dtype=np.float64), p[m].shape).copy(), np.full(int(m.sum()), 1e300)).astype(bool)
                for v in case.lights]
    orc.close()
    print(f"{name}: {int(m.sum())} of {WID * HGT} pixels hit, shadowed per light {[int(s.sum()) for s in shadowed]}")
    assert m.sum() >= 0.1 * WID * HGT and (~m).sum() >= 32
    if case.shadows:
        assert shadowed[0].sum() >= 32
    else:
        assert not any(s.any() for s in shadowed)
    assert (~np.all(shadowed, axis=0)).sum() >= 32, "no hits that some light reaches"


def test_the_meshes_have_the_structures_the_cases_name():
    """blob(7): no pairs (and no tree: see CASES), blob(8): the smallest with a grid; concentric: cells of more
    than 64 entries (a second chunk in mesh_shadow_grid); two_clusters under this light and identical: a tree and no grid."""
    def first_pair(name):
        pairs, nodes, _, leaf_pairs = S.mesh_structures(CASES[name].mesh, [tuple(float(x) for x in v) for v in CASES[name].lights])
        return (None if int(leaf_pairs[0]) == 0xFFFFFFFF else pairs[int(leaf_pairs[0])]), nodes
    assert first_pair("blob(7)")[0] is None
    rec, _ = first_pair("blob(8)")
    assert rec is not None and grid_of(rec)[2] > 0
    rec, nodes = first_pair("concentric")
    assert grid_of(rec)[2] > 0 and (S.cell_counts(rec, nodes) > 64).any()
    for name in ("two_clusters", "identical"):
        rec, _ = first_pair(name)
        assert rec is not None and grid_of(rec)[2] == 0, name
    assert {c.spp for c in CASES.values()} == {2, 4, 16, 32}
    assert {len(c.lights) for c in CASES.values()} >= {1, 3} and any(HAIR in c.lights for c in CASES.values())


# =============================================================================================================================
# GPU half

def ran_between(before, after):
    return {k: after[k] - before[k] for k in after}


def on_off(ctx, render, expect_new):
    """render() with primary_mesh_kernel 1, 0, 1: the same bits and counters; the new kernel took every bounce-0 launch of the frames with
    the option on iff expect_new, and none with it off.  Returns the frame and the counters."""
    out = []
    try:
        for opt in (1, 0, 1):
            ctx.set_option("primary_mesh_kernel", opt)
            before = ctx.primary_kernels()
            img, st = render()
            ran = ran_between(before, ctx.primary_kernels())
            if opt and expect_new:
                assert ran["k_primary_mesh"] > 0 and ran["k_primary"] == 0, ran
            else:
                assert ran["k_primary_mesh"] == 0, ran
            out.append((img, counters(st) if st is not None else None))
    finally:
        ctx.set_option("primary_mesh_kernel", 1)
    for k in (0, 2):
        assert np.array_equal(out[1][0], out[k][0]), f"frames differ on {np.count_nonzero(np.any(out[1][0] != out[k][0], axis=-1))} pixels"
    assert out[1][1] == out[2][1]                                    # (a scene's first frame launches every reflection level: the second and third are compared)
    return out[2]


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_bare_mesh(hip, name):
    case = CASES[name]
    cam, jit = camera_of(case), ft.jitter_pattern(case.spp)
    lower_of(case)(hip)
    frame, st = on_off(hip, lambda: hip.render(cam, WID, HGT, case.spp, jit), expect_new=case.qualifies)
    H.assert_frames_match(frame, oracle_frame(name), what=name)
    assert st["hits_primary"] > 0 and st["rays_shadow"] == len(case.lights) * st["hits_primary"] and st["csg_overflow"] == 0
    L = hip.block_lists()
    if name in ("identical", "concentric"):                          # 300 / 200 triangles around one centre: every block sees more than 64 candidates and walks the tree
        assert L["leaf"] == 0 and (L["heads"] == _capi.LIST_NONE).all()
    elif case.qualifies:
        assert L["leaf"] == 0 and (L["heads"] != _capi.LIST_NONE).any()
    else:
        assert L["leaf"] == -1                                       # no tree: no lists either


@gpu
def test_unlit_material_takes_k_primary(hip):
    """shadeIfRequired (Shading.fs:100-104): the leaf of an unlit material is not lit, which the kernel is not written for."""
    case = CASES["blob(65)"]
    lower = lower_mesh(tris_of(case), case.ops, case.lights, case.material, unlit=True)
    cam, jit = camera_of(case), ft.jitter_pattern(4)
    lower(hip)
    frame, st = on_off(hip, lambda: hip.render(cam, WID, HGT, 4, jit), expect_new=False)
    orc = O.Oracle()
    lower(orc)
    H.assert_frames_match(frame, orc.render(cam, WID, HGT, 4, jit)[0], what="unlit")
    assert st["hits_primary"] > 0 and st["rays_shadow"] == 0


@gpu
def test_every_combination_of_the_three_options_gives_one_frame(hip):
    case = CASES["blob(65)"]
    cam, jit = camera_of(case), ft.jitter_pattern(case.spp)
    lower, got = lower_of(case), []
    try:
        for lists in (0, 1):
            for lss in (0, 1, 2):
                hip.set_option("primary_block_lists", lists)
                hip.set_option("light_space_shadows", lss)
                lower(hip)
                got.append(on_off(hip, lambda: hip.render(cam, WID, HGT, case.spp, jit), expect_new=True))
                assert (hip.block_lists()["leaf"] == 0) == bool(lists)
    finally:
        hip.set_option("primary_block_lists", 1)
        hip.set_option("light_space_shadows", 2)
    for frame, st in got:
        assert np.array_equal(frame, got[0][0]) and st == got[0][1]
    H.assert_frames_match(got[0][0], oracle_frame("blob(65)"), what="options")


def _ball(b):
    return [b.material(b.transform([("scale", (0.05, 0.05, 0.05)), ("translate", (-0.9, -1.1, 0.1))], b.primitive(ft.SPHERE)), colour=(0.3, 0.8, 0.4))]


def _focus(cam):
    cam.has_focus, cam.focal_length, cam.aperture_angular_size = 1, 0.25, H.deg(0.5)
    return cam


# what disqualifies: name -> (lower_mesh keywords, context options, spp, camera change)
FALLBACKS = {
    "second item": (dict(extra=_ball), {}, 4, None),
    "point light": (dict(point=(-1.5, -0.5, 0.3)), {}, 4, None),
    "bspMesh 2": (dict(depth=2), {}, 4, None),
    "reflective": (dict(material=dict(colour=(0.8, 0.7, 0.6), reflectance=0.5)), {}, 4, None),
    "focus camera": ({}, {}, 4, _focus),
    "coherent_waves = 0": ({}, {"coherent_waves": 0}, 4, None),
    "uniform_surface = 0": ({}, {"uniform_surface": 0}, 4, None),
    "plain numbering": ({}, {}, 3, None),
}


@gpu
@pytest.mark.parametrize("what", list(FALLBACKS))
def test_what_the_kernel_is_not_written_for_takes_k_primary(hip, what):
    case = CASES["blob(65)"]
    kw, opts, spp, change = FALLBACKS[what]
    args = dict(ops=case.ops, lights=case.lights[:1], material=case.material)
    args.update(kw)
    lower = lower_mesh(tris_of(case), **args)
    cam, jit = camera_of(case), ft.jitter_pattern(spp)
    if change:
        cam = change(cam)
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        lower(hip)
        frame, st = on_off(hip, lambda: hip.render(cam, WID, HGT, spp, jit), expect_new=False)
    finally:
        for k in opts:
            hip.set_option(k, 1)
    orc = O.Oracle()
    lower(orc)
    H.assert_frames_match(frame, orc.render(cam, WID, HGT, spp, jit)[0], what=what)
    assert st["hits_primary"] > 0


@gpu
def test_progressive_passes_and_aov_take_k_primary(hip, blocking):
    case = CASES["blob(65)"]
    cam, jit = camera_of(case), ft.jitter_pattern(4)
    lower_of(case)(hip)

    def two_passes():
        hip.progressive_begin(cam, WID, HGT)
        try:
            hip.progressive_pass(4, jit, seed=1)
            return hip.progressive_pass(4, jit, seed=2)
        finally:
            hip.progressive_end()
    on_off(hip, two_passes, expect_new=False)

    def aov():
        a = hip.render_aov(cam, WID, HGT, 4, jit, sample=1, channels=["t", "leaf", "triangle"])
        return np.stack([a["t"], a["leaf"].astype(np.float64), a["triangle"].astype(np.float64)], axis=-1), None
    before = hip.primary_kernels()
    on_off(hip, aov, expect_new=False)
    assert hip.primary_kernels() == before                           # (k_aov is no bounce-0 launch at all)
    # and the plain frame of the same scene still takes the new kernel afterwards
    frame, _ = on_off(hip, lambda: hip.render(cam, WID, HGT, case.spp, ft.jitter_pattern(case.spp)), expect_new=True)
    assert np.array_equal(frame, blocking["held"][0])


def _views(kind):
    case = CASES["blob(65)"]
    eye = np.array(case.eye)
    return [ft.make_camera(tuple(eye + (0.0 if kind == "held" else 0.01 * k) * np.array([0.3, -0.2, 0.1])), case.look, (0, 1, 0), math.radians(case.fov), WID / HGT) for k in range(5)]


@pytest.fixture(scope="module")
def blocking(hip):
    """Five blocking frames of blob(65), camera held and camera moving, with the option 0: what the queued frames must equal."""
    case = CASES["blob(65)"]
    jit = ft.jitter_pattern(case.spp)
    lower_of(case)(hip)
    hip.set_option("primary_mesh_kernel", 0)
    try:
        return {kind: [hip.render(cam, WID, HGT, case.spp, jit)[0] for cam in _views(kind)] for kind in ("held", "moving")}
    finally:
        hip.set_option("primary_mesh_kernel", 1)


@gpu
@pytest.mark.parametrize("kind", ["held", "moving"])
@pytest.mark.parametrize("reuse", [1, 0], ids=["classify_reuse", "classify_again"])
def test_queued_frames_equal_the_blocking_ones(hip, blocking, kind, reuse):
    """Five frames queued back to back (two main streams: two in flight), each copied out behind its last kernel.  With classify_reuse the
    held view's later frames find their slot's classification warm, without it every frame classifies: the same frames."""
    case = CASES["blob(65)"]
    jit = ft.jitter_pattern(case.spp)
    lower_of(case)(hip)
    outs = [ft.PinnedArray((HGT, WID, 3)) for _ in range(5)]
    try:
        hip.set_option("classify_reuse", reuse)
        for rounds in range(2):                                      # the second round of the held view starts warm in every slot
            before = hip.primary_kernels()
            for cam, out in zip(_views(kind), outs):
                out.array[:] = 0
                hip.render_enqueue(cam, WID, HGT, case.spp, jit, out=out.array)
            st = hip.wait()
            ran = ran_between(before, hip.primary_kernels())
            assert ran["k_primary_mesh"] >= 5 and ran["k_primary"] == 0, ran
            for k, out in enumerate(outs):
                assert np.array_equal(out.array, blocking[kind][k]), (kind, reuse, rounds, k)
            assert st["hits_primary"] > 0
    finally:
        hip.set_option("classify_reuse", 1)
        for out in outs:
            out.close()
    H.assert_frames_match(blocking["held"][0], oracle_frame("blob(65)"), what="queued")


@gpu
def test_headline_scene(hip):
    p = ft.parse_scene_file(H.scene_path("bunny"))
    p.lower(hip)
    jit = ft.jitter_pattern(16)
    frame, st = on_off(hip, lambda: hip.render(p.camera, 64, 40, 16, jit), expect_new=True)
    orc = O.Oracle()
    p.lower(orc)
    H.assert_frames_match(frame, orc.render(p.camera, 64, 40, 16, jit)[0], what="bunny")
    assert st["rays_shadow"] > 0

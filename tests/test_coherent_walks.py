"""The mesh walks of coherent waves, per ray, against the oracle and against their per-lane twins.

trace() (ft_kernels.hip) sends a mesh query down one of six walks.  Context.closest / blocked trace with coherent = false, so every
ray-exact test elsewhere in the suite reaches the two per-lane walks only (mesh_bvh_query, mesh_bsp_query).  Here the rays are the
pixels of a pinhole frame: render_aov runs the coherent closest walk for each (mesh_bsp_packet, mesh_bsp_narrow, mesh_bvh_packet) and
returns t, p, n, leaf and triangle per pixel, the oracle's ray_through_pixel + slightOffset rebuilds the same rays on the CPU, and the
option coherent_waves = 0 sends the very same pixels down the per-lane walks as a second witness.  Per case:

  1. planes against the oracle's closest() under helpers.assert_hits_match;
  2. planes of coherent_waves 1 and 0: hit mask, leaf, node and triangle identical, t bitwise equal;
  3. a frame under a directional and a point light with light_space_shadows = 0 and primary_block_lists = 0 (the tree walks themselves
     answer the shadow rays): bitwise its coherent_waves = 0 twin, and the oracle's frame at 1e-4 with the worst pixel under 1e-6;
     the eye and the light are chosen per mesh so that hits are shadowed before the light and others only beyond it, which the CPU half
     counts on the oracle (walk_tools names the meshes that cannot give that);
  4. once per mesh family, the same frame with the default options (grids, lists): bitwise again.

The cases (tests/walk_tools.py): the record shapes of shallow BSPs (eleven catalogue meshes at bspMesh 1, 2, 3, 5; from outside, from
inside the box, under rotate + non-uniform scale; frames 76 and 52 wide, a tile list that hangs over the frame's edge), trees of 40 and
41 levels (the first with two-level records, the second without), trees of 63 .. 66 levels (up to and past the 64 entries of a WaveStack),
right-deep and left-deep, and cameras whose centre column and row of rays are exactly parallel to a model axis.

The first half needs no GPU: it proves on a host-only context and the oracle that the scenes are what they claim."""
import numpy as np
import pytest

import functracer_amd as ft

from . import bvh_tools as B
from . import helpers as H
from . import walk_tools as W

gpu = pytest.mark.gpu
PLANES = ["t", "p", "n", "colour", "leaf", "node", "triangle"]
SHALLOW_CASES = [(name, depth) for name in W.SHALLOW for depth in W.SHALLOW_DEPTHS]
TALL_CASES = [(n, sign) for n in W.TALL_SIZES for sign in (1, -1)]
TALL_DEPTH = 200                                                    # bspMesh 200: the tree ends where the triangles do


def _tall_id(c):
    return f"{c[0]}{'+' if c[1] > 0 else '-'}"


def _host_trees(tris, depth, ops=None):
    ctx = ft.Context(host_only=True)
    W.build(ctx, tris, depth, ops)
    T, info = ctx.mesh_trees(), ctx.scene_info()
    ctx.close()
    return T, info


# =============================================================================================================================
# CPU half

@pytest.mark.parametrize("n,sign", TALL_CASES, ids=[_tall_id(c) for c in TALL_CASES])
def test_tall_meshes_are_as_tall_as_they_claim(n, sign):
    """n triangles: n - 1 branch levels, a per-lane stack of n entries; two-level records up to 40 levels and none beyond; the right
    spine - what a walk that descends right keeps pending - is the whole height for sign +1 and one node for sign -1."""
    T, info = _host_trees(W.tall(n, sign), TALL_DEPTH)
    assert W.bsp_height(T) == n - 1
    assert T["stack_capacity"] == n == info["stack_capacity"]
    assert info["bsp_leaves"] == n and info["triangles"] == n, "one triangle per leaf, none clipped"
    assert W.right_spine(T) == (n - 1 if sign > 0 else 1)
    wide = int(T["meshes"][0][3])
    assert (wide != W.INT32_MIN) == (n - 1 <= W.PACKET_LEVELS)
    if wide != W.INT32_MIN:                                         # 40 levels: 20 records, each with one leaf beside an absent sibling
        recs = W.wide_records(T)
        assert len(recs) == (n - 1) // 2 and all(c.count(W.INT32_MIN) >= 1 for c in recs)


def test_flattener_gives_160_and_161_stack_entries_for_159_and_160_levels():
    """The two scenes of test_lds_refusal_on_the_device, on the flattener alone.  A host-only context launches nothing and never refuses
    for LDS (ft_capi.cpp, commit_scene): it takes both; the refusal is the device test's to observe."""
    for n in (W.LDS_STACK_ENTRIES, W.LDS_STACK_ENTRIES + 1):
        T, info = _host_trees(W.tall(n, 1) * 3.0 ** -94, TALL_DEPTH)               # (scaled down: 3^160 is past the float cull records)
        assert info["stack_capacity"] == n and W.bsp_height(T) == n - 1


def test_shallow_cases_hold_the_record_shapes():
    """Across the shallow set: a record with a leaf child beside an absent sibling (the leaf takes the first slot of its half, the
    second is INT32_MIN), a record with four branch grandchildren, a root whose two children are leaves, odd heights, and single-leaf
    roots (identical, concentric: every cut clips every triangle, BspMesh.fs:59-60), which take the BVH walks at every depth."""
    seen = {"leaf_beside_absent": 0, "four_branches": 0, "two_leaf_root": 0, "odd_height": 0, "single_leaf_root": 0, "clipped": 0}
    for name, depth in SHALLOW_CASES:
        e = B.catalogue()[name]
        T, info = _host_trees(e.tris, depth)
        root, height = int(T["meshes"][0][0]), W.bsp_height(T)
        assert height <= depth
        if root < 0:
            assert name in ("identical", "concentric"), name
            seen["single_leaf_root"] += 1
            continue
        recs = W.wide_records(T)
        assert recs, (name, depth)
        for ch in recs:
            for half in (ch[0:2], ch[2:4]):
                assert half[0] != W.INT32_MIN, "the first slot of a half is never empty"
                seen["leaf_beside_absent"] += half[0] < 0 and half[1] == W.INT32_MIN
            seen["four_branches"] += all(c >= 0 for c in ch)
        seen["two_leaf_root"] += recs[0][1] == W.INT32_MIN and recs[0][3] == W.INT32_MIN and recs[0][0] < 0 and recs[0][2] < 0
        seen["odd_height"] += height % 2
        seen["clipped"] += info["triangles"] > e.tris.shape[0]
    assert all(v > 0 for v in seen.values()), seen
    assert seen["single_leaf_root"] == 2 * len(W.SHALLOW_DEPTHS)


@pytest.mark.parametrize("name,depth", W.AXIS_CASES)
def test_axis_views_hold_exactly_axis_parallel_rays(name, depth):
    """The mesh stands under no transform, so model space is world space: one pixel column's rays have x = 0.0 and one pixel row's have
    y = 0.0, exactly, and every 8x8 block those cross is a wave with such a lane; and some of those rays hit."""
    ref = W.reference("axis", name, depth, "axis")
    d, hit = ref["d"], ref["closest"][0].astype(bool)
    for axis in (0, 1):
        zero = d[:, axis] == 0.0
        assert zero.sum() == ref["view"].w and (d[zero, 2] != 0.0).all(), (axis, int(zero.sum()))
        assert hit[zero].any(), "an axis-parallel ray hits the mesh"
    assert ((d[:, 0] == 0.0) & (d[:, 1] == 0.0)).sum() == 1        # the centre ray: parallel to z itself
    assert 0.05 < hit.mean() < 0.9                                  # (the field of view is part of what makes the zeros exact: no zooming here)


@pytest.mark.parametrize("name,depth", SHALLOW_CASES)
def test_shallow_views_are_alive_on_the_oracle(name, depth):
    for view in W.shallow_views(name):
        ref = W.reference("shallow", name, depth, view.name)
        share = float(ref["closest"][0].mean())
        assert 0.1 < share < 0.9, (name, view.name, share)
        if view.name == "inside":                                   # entry distance < 0: the eye is strictly inside the root's box
            lo, hi = ref["tris"].reshape(-1, 3).min(axis=0), ref["tris"].reshape(-1, 3).max(axis=0)
            assert ((view.o > lo) & (view.o < hi)).all()


@pytest.mark.parametrize("name,depth", SHALLOW_CASES)
def test_shallow_shadow_frames_hold_shadows(name, depth):
    """On the oracle, for the view and the light of every shadow frame: primary hits with an occluder before the point light, hits with one
    only beyond it, and hits in the open.  The meshes that cannot give that are named in walk_tools, and shown here to be what they are called."""
    ref = W.reference("shallow", name, depth, "shadow")
    hits, near, far = W.shadow_counts(ref, depth)
    assert hits >= 0.08 * len(ref["xs"]), (hits, near, far)
    if name in W.NO_SELF_SHADOW:
        assert near == far == 0
    elif name in W.BEFORE_ONLY:
        assert 100 <= near < hits - 100, (hits, near, far)
    else:
        assert near >= 30 and far - near >= 30 and hits - far >= 30, (hits, near, far)


@pytest.mark.parametrize("name,depth", [c for c in W.AXIS_CASES if c[0] != "flat"])
def test_axis_shadow_frames_hold_shadows(name, depth):
    """(`flat` cannot shadow itself: walk_tools.NO_SELF_SHADOW.)"""
    hits, near, far = W.shadow_counts(W.reference("axis", name, depth, "axis"), depth)
    assert 0 < near < far < hits, (hits, near, far)


@pytest.mark.parametrize("n,sign", TALL_CASES, ids=[_tall_id(c) for c in TALL_CASES])
def test_tall_views_are_alive_on_the_oracle(n, sign):
    """Every view shows at least two triangles, that is two leaves; the small-end view shows triangles 1 and 2, which hang at the levels
    n - 2 and n - 3: the deepest left leaves of the right-deep tree, beyond entry 64 of a wave stack from 66 triangles on."""
    for view in W.tall_views(n, sign):
        ref = W.reference("tall", (n, sign), TALL_DEPTH, view.name)
        hit, _, p = ref["closest"][0].astype(bool), ref["closest"][1], ref["closest"][2]
        seen = set(W.tall_triangle_of(p[hit]).tolist())
        assert len(seen) >= 2 and hit.mean() > 0.1, (view.name, sorted(seen), hit.mean())
        if view.name == "small":
            assert {1, 2, 3} <= seen, sorted(seen)
            for k in (1, 2):
                assert (W.tall_triangle_of(p[hit]) == k).sum() >= 40, f"triangle {k} fills too little of the frame"
            hits, near, far = W.shadow_counts(ref, TALL_DEPTH)       # the point light: occluders before it, more beyond it, and lit hits
            assert 0 < near < far < hits and far - near >= 100, (hits, near, far)
        else:
            assert {n - 1, n - 2, n - 3} <= seen, sorted(seen)


# =============================================================================================================================
# GPU half

# A context of the module's own, not the session's `hip`: the tests switch coherent_waves, primary_block_lists and the commit-time
# light_space_shadows, and a test that fails between a switch and its restore must not leave the rest of the suite under other options.
@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    yield c
    c.close()


def _aov(ctx, view, coherent):
    ctx.set_option("coherent_waves", coherent)
    try:
        return ctx.render_aov(W.camera(view), view.w, view.h, 1, np.zeros((1, 2)), tiles=view.tiles, channels=PLANES)
    finally:
        ctx.set_option("coherent_waves", 1)


def _check_planes(ctx, kind, name, depth, view_name):
    """Points 1 and 2 of the module docstring for one view."""
    ref = W.reference(kind, name, depth, view_name)
    view, xs, ys = ref["view"], ref["xs"], ref["ys"]
    what = f"{kind} {name} bspMesh {depth} {view_name}"
    W.build(ctx, ref["tris"], depth, view.ops, ref["light"])
    co, inco = _aov(ctx, view, 1), _aov(ctx, view, 0)
    whit = ref["closest"][0]
    for got, route in ((co, "coherent"), (inco, "per-lane")):
        ghit = (got["leaf"][ys, xs] >= 0).astype(np.int32)
        print(f"{what} {route}: {int(ghit.sum())} hits of {len(xs)} rays, oracle {int(whit.sum())}")
        H.assert_hits_match((ghit, got["t"][ys, xs], got["p"][ys, xs], got["n"][ys, xs], got["colour"][ys, xs]), ref["closest"], what=f"{what} {route}")
        assert got["stats"]["rays_primary"] == len(xs) and got["stats"]["hits_primary"] == int(whit.sum())
        if view.tiles is not None:                                  # nothing outside the tiles was written
            outside = np.ones((view.h, view.w), bool)
            outside[ys, xs] = False
            assert (got["leaf"][outside] == -1).all() and np.isinf(got["t"][outside]).all()
    for k in ("leaf", "node", "triangle"):
        diff = co[k] != inco[k]
        assert not diff.any(), f"{what}: plane {k} differs between the routes on {int(diff.sum())} pixels, first {np.argwhere(diff)[:3].tolist()}"
    tdiff = co["t"].view(np.uint64) != inco["t"].view(np.uint64)
    assert not tdiff.any(), f"{what}: t differs in its bits on {int(tdiff.sum())} pixels, by up to {np.nanmax(np.abs(co['t'][tdiff] - inco['t'][tdiff]) / np.spacing(np.abs(inco['t'][tdiff]))):.0f} ulp"
    return co


def _frames(ctx, kind, name, depth, view_name, w, h):
    """Point 3: the frame with the tree walks answering every query, both routes, against the oracle's; returns the frame."""
    view, light, tris, want = W.reference_frame(kind, name, depth, view_name, w, h)
    what = f"{kind} {name} bspMesh {depth} {view_name} frame"
    jit = ft.jitter_pattern(2)
    ctx.set_option("light_space_shadows", 0)
    ctx.set_option("primary_block_lists", 0)
    try:
        W.build(ctx, tris, depth, view.ops, light)
        co, st = ctx.render(W.camera(view), w, h, 2, jit)
        ctx.set_option("coherent_waves", 0)
        inco, st0 = ctx.render(W.camera(view), w, h, 2, jit)
    finally:
        ctx.set_option("coherent_waves", 1)
        ctx.set_option("light_space_shadows", 2)
        ctx.set_option("primary_block_lists", 1)
    diff = np.any(co != inco, axis=2)
    assert not diff.any(), f"{what}: the two routes differ on {int(diff.sum())} pixels, first {np.argwhere(diff)[:3].tolist()}"
    assert st["rays_shadow"] == st0["rays_shadow"] and st["rays_shadow"] > 0
    assert not np.isnan(co).any()
    worst = H.assert_frames_match(co, want, what=what)
    print(f"{what}: worst pixel {worst:.3e}")
    assert worst < 1e-6, f"{what}: worst pixel {worst:.3e}"
    lit = (want.sum(axis=2) > 0).mean()                             # (what stands in shadow: test_*_shadow_frames_hold_shadows, on the oracle)
    assert lit > 0.05, f"{what}: {lit:.3f} of the frame is lit"
    return co, (view, light, tris, jit)


def _check_defaults(ctx, frame, scene, depth, w, h):
    """Point 4: grids and lists back on, the same frame bit for bit."""
    view, light, tris, jit = scene
    W.build(ctx, tris, depth, view.ops, light)
    got, _ = ctx.render(W.camera(view), w, h, 2, jit)
    diff = np.any(got != frame, axis=2)
    assert not diff.any(), f"default options move {int(diff.sum())} pixels"


@gpu
@pytest.mark.parametrize("name,depth", SHALLOW_CASES)
def test_shallow_bsp_planes(ctx, name, depth):
    for view in W.shallow_views(name):
        _check_planes(ctx, "shallow", name, depth, view.name)


@gpu
@pytest.mark.parametrize("name,depth", SHALLOW_CASES)
def test_shallow_bsp_shadows(ctx, name, depth):
    frame, scene = _frames(ctx, "shallow", name, depth, "shadow", 60, 52)
    if depth == 3:                                                  # once per mesh
        _check_defaults(ctx, frame, scene, depth, 60, 52)


@gpu
@pytest.mark.parametrize("n,sign", TALL_CASES, ids=[_tall_id(c) for c in TALL_CASES])
def test_tall_tree_planes(ctx, n, sign):
    for view in W.tall_views(n, sign):
        co = _check_planes(ctx, "tall", (n, sign), TALL_DEPTH, view.name)
        assert len(np.unique(co["triangle"][co["triangle"] >= 0])) >= 2


@gpu
@pytest.mark.parametrize("n,sign", TALL_CASES, ids=[_tall_id(c) for c in TALL_CASES])
def test_tall_tree_shadows(ctx, n, sign):
    """The small end only: the shadow ray starts 1e-4 off the surface (Shading.fs:109-117), which at the large end, where a coordinate's
    last bit is worth 1e14, is no offset at all - whether a surface there shadows itself is rounding, not a walk."""
    frame, scene = _frames(ctx, "tall", (n, sign), TALL_DEPTH, "small", 52, 44)
    if n in (41, 66):
        _check_defaults(ctx, frame, scene, TALL_DEPTH, 52, 44)


@gpu
@pytest.mark.parametrize("name,depth", W.AXIS_CASES)
def test_axis_parallel_lanes(ctx, name, depth):
    _check_planes(ctx, "axis", name, depth, "axis")
    frame, scene = _frames(ctx, "axis", name, depth, "axis", 60, 60)
    _check_defaults(ctx, frame, scene, depth, 60, 60)


@gpu
def test_lds_refusal_on_the_device(ctx):
    """159 levels fill the 160 KiB exactly and render; 160 levels are refused with the LDS message, and the scene before stays."""
    small = W.tall_views(95, 1)[0]._replace(w=36, h=28)             # beside the triangle of size 1: number 94 of the scaled mesh
    for n in (W.LDS_STACK_ENTRIES, W.LDS_STACK_ENTRIES + 1):
        tris = W.tall(n, 1) * 3.0 ** -94
        if n == W.LDS_STACK_ENTRIES:
            W.build(ctx, tris, TALL_DEPTH)
            assert ctx.scene_info()["stack_capacity"] == n
            want = ctx.render_aov(W.camera(small), small.w, small.h, 1, np.zeros((1, 2)), channels=["t", "triangle"])
            assert len(np.unique(want["triangle"])) >= 3
            continue
        with pytest.raises(ft.FtError) as e:
            W.build(ctx, tris, TALL_DEPTH)
        assert e.value.status == -4 and "more than 160 KiB of LDS per workgroup for CSG lists / BSP stacks" in str(e.value), str(e.value)
        again = ctx.render_aov(W.camera(small), small.w, small.h, 1, np.zeros((1, 2)), channels=["t", "triangle"])
        assert np.array_equal(again["triangle"], want["triangle"]) and np.array_equal(again["t"], want["t"])

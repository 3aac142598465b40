"""Option "edge_cull" (functracer_amd/csrc/ft_edges.h): beside its rectangle every entry of a block's candidate list and of
a shadow grid carries the three edges of its projected triangle, and a wavefront whose rectangle lies wholly outside one of them skips
the triangle.

CPU: the numpy twin of the record and of the wave test (tests/edge_tools.py) on the hard-mesh catalogues of tests/list_tools.py (the
cases of test_block_lists_exact) and tests/shadow_tools.py, under random batch rectangles, against an exact triangle-against-rectangle
test in longdouble: a triangle that a ray of the rectangle can hit is never dropped; and a view and a light in which the edges keep at
least a quarter fewer entries than the rectangles.

GPU: the records read back (Context.edge_records) hold their exact triangles, cut off the point 1 % of the triangle's size beyond each
edge's midpoint, and are the sentinel exactly where the rule says; frames and every counter with the option 0 and 1 are equal bit for bit
on the catalogues and the bunny, under one and three lights, with the mesh kernel, the lists and the grids on and off, on queued frames that
reuse a slot's lists, after ft_scene_commit_lights and ft_scene_commit_deformed and through a two-device context; a few of those frames
are compared with the oracle's."""
import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import edge_tools as E
from . import helpers as H
from . import list_tools as LT
from . import shadow_tools as ST
from . import walk_tools as W
from . import test_block_lists_exact as LX
from .test_block_lists import counters
from .test_classify_reuse import CAM_A, CAM_B, TRIS, bunny_ops
from .test_light_space_shadows import light_space

LD = LT.LD
# the list cases whose rectangles mean something (the others assert their outcome in test_block_lists_exact) and that are quick to refer
LIST_CASES = [n for n in LX.NAMES if LX.CASES[n].expect not in LX.EXEMPT and n != "pool"]
RECORD_CASES = ["blob(65)-out", "blob(1025)-in", "concentric-in", "flat-1e-9-above", "spanning-out", "degenerate-out", "geometric-near", "plane-a=0", "plane-in-triangle",
                "xf-sliver", "xf-mirror", "fov-150", "tiny-stacks", "jitter-3.5"]
GRID_CASES = [n for n in ST.SINGLE if n not in ("identical",)]
THREE_LIGHTS = [(-3, -2, 3), (2, -3, 1), (0.5, -1, -2)]


def _twin_of_list_case(name):
    c, ref = LX.CASES[name], LX.ref_of(name)
    jx, jy, infl, bounded = E.list_inputs(ref, c.tris, c.ops, c.cam)
    with np.errstate(invalid="ignore"):
        rec, info = E.edge_records(np.where(bounded[:, None], jx, 0).astype(np.float64), np.where(bounded[:, None], jy, 0).astype(np.float64), infl, bounded)
    return ref, jx, jy, bounded, rec, info


def _kept(rec, x, y, rng, n, spread):
    """Random rectangles around the triangles x, y, rounded outward to float: (overlaps by the exact test, of those the twin keeps, what
    the rectangles alone keep, what the twin keeps of those)."""
    t, x0, x1, y0, y1 = E.random_rects(rng, x, y, n, spread)
    f0, f1, g0, g1 = LT.float_below(x0.astype(LD)), LT.float_above(x1.astype(LD)), LT.float_below(y0.astype(LD)), LT.float_above(y1.astype(LD))
    hit = E.exact_overlap(x[t], y[t], x0, x1, y0, y1)
    out = E.wave_outside(rec[t], f0, f1, g0, g1)
    xs, ys = np.asarray(x, dtype=np.float64)[t], np.asarray(y, dtype=np.float64)[t]
    in_rect = (xs.min(axis=1) <= f1) & (xs.max(axis=1) >= f0) & (ys.min(axis=1) <= g1) & (ys.max(axis=1) >= g0)
    return hit, out, in_rect


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_twin_and_exact_test_on_hand_worked_triangles():
    x, y = np.array([[0.0, 4.0, 0.0]]), np.array([[0.0, 0.0, 3.0]])
    rec, info = E.edge_records(x, y, 1e-3)
    assert not E.is_sentinel(rec)[0]
    # the hypotenuse 3 x + 4 y = 12: unit normal (0.6, 0.8), c = -(2.4 + margin)
    hyp = rec[0, 1]
    assert abs(hyp[0] - 0.6) < 1e-6 and abs(hyp[1] - 0.8) < 1e-6 and -2.4 - 3e-3 < hyp[2] < -2.4 - 1.4e-3
    assert E.assert_records_hold(rec, x, y, "3-4-5") == 1
    for rect, overlap in (((3.0, 3.2, 2.0, 2.2), False), ((1.9, 2.1, 1.4, 1.6), True), ((-0.2, -0.1, 1.0, 1.1), False), ((1.0, 1.1, 1.0, 1.1), True)):
        assert bool(E.exact_overlap(x, y, *rect)[0]) is overlap
        assert bool(E.wave_outside(rec, *rect)[0]) is (not overlap)
    # the bounding rectangle holds (3, 2.2) - the rectangle test keeps it - and the hypotenuse drops it
    assert 0 <= 3.0 <= 4 and 0 <= 2.2 <= 3 and E.wave_outside(rec, 3.0, 3.2, 2.0, 2.2)[0]
    # sentinels: a sliver, a point, an unbounded rectangle, a triangle lost in its coordinates, a NaN; and what they never do
    sl, _ = E.edge_records(np.array([[0.0, 1.0, 0.5]]), np.array([[0.0, 0.0, 1e-7]]), 0.0)
    pt, _ = E.edge_records(np.array([[1.0, 1.0, 1.0]]), np.array([[2.0, 2.0, 2.0]]), 0.0)
    ub, _ = E.edge_records(x, y, 1e-3, bounded=[False])
    far, _ = E.edge_records(x * 1e-6 + 1e3, y * 1e-6 + 1e3, 0.0)
    nan, _ = E.edge_records(np.array([[0.0, np.nan, 0.0]]), y, 0.0)
    for r in (sl, pt, ub, far, nan):
        assert E.is_sentinel(r)[0] and not E.wave_outside(r, 1e6, 2e6, 1e6, 2e6)[0]
    assert not E.wave_outside(rec, np.nan, 1.0, 0.0, 1.0)[0] and not E.wave_outside(rec, -np.inf, np.inf, -np.inf, np.inf)[0]


@pytest.mark.parametrize("name", LIST_CASES)
def test_twin_keeps_every_list_triangle_a_rectangle_can_reach(name):
    ref, jx, jy, bounded, rec, info = _twin_of_list_case(name)
    assert E.is_sentinel(rec[~bounded]).all()
    b = np.nonzero(bounded)[0]
    if b.size == 0:
        return
    rng = np.random.default_rng(20260101)
    x, y = jx[b], jy[b]
    for spread in (0.3, 1.0):
        hit, out, _ = _kept(rec[b], x, y, rng, 24, spread)
        bad = hit & out
        assert not bad.any(), f"{name}: {int(bad.sum())} rectangles that overlap their triangle are dropped by its record"
    E.assert_records_hold(rec[b], x, y, name)


@pytest.mark.parametrize("name", GRID_CASES)
def test_twin_keeps_every_grid_triangle_a_rectangle_can_reach(name):
    pairs, nodes, tris, _ = ST.structures(name)
    rng = np.random.default_rng(20260102)
    grids = 0
    for _, P in ST.pairs_of(name):
        k = int(np.nonzero((pairs == P).all(axis=1))[0][0])
        idx, x, y, boxes = E.grid_entries(pairs, nodes, tris, k)
        if idx.size == 0:
            continue
        grids += 1
        sel = rng.choice(idx.size, size=min(idx.size, 4000), replace=False)
        x, y, boxes = x[sel], y[sel], boxes[sel]
        infl = E.grid_inflation(x, y, boxes)
        assert (infl >= 0).all()
        rec, info = E.edge_records(x.astype(np.float64), y.astype(np.float64), infl)
        for spread in (0.3, 1.0):
            hit, out, _ = _kept(rec, x, y, rng, 8, spread)
            bad = hit & out
            assert not bad.any(), f"{name}: {int(bad.sum())} rectangles that overlap their triangle are dropped by its record"
        E.assert_records_hold(rec, x, y, name)
    if name in ("blob(65)", "blob(1025)", "degenerate", "spanning", "geometric", "flat-off-plane"):   # (the cases of test_grid_records_on_the_device)
        assert grids > 0, name


def test_edges_keep_a_quarter_fewer_entries_than_the_rectangles():
    """A view (blob(65) from outside, 64 x 48) and a light (blob(65), the general direction) under batch footprints a twentieth of a
    triangle wide: what the rectangles keep and what the edges keep of it."""
    print()
    rng = np.random.default_rng(20260103)
    ref, jx, jy, bounded, rec, _ = _twin_of_list_case("blob(65)-out")
    b = np.nonzero(bounded)[0]
    _, out, in_rect = _kept(rec[b], jx[b], jy[b], rng, 200, 0.6)
    by_rect, by_edges = int(in_rect.sum()), int((in_rect & ~out).sum())
    print(f"  lists, blob(65)-out: the rectangles keep {by_rect}, the edges {by_edges} ({by_edges / by_rect:.3f})")
    assert by_rect > 1000 and by_edges <= 0.75 * by_rect
    pairs, nodes, tris, _ = ST.structures("blob(65)")
    k = int(np.nonzero((pairs == ST.pairs_of("blob(65)")[0][1]).all(axis=1))[0][0])
    idx, x, y, boxes = E.grid_entries(pairs, nodes, tris, k)
    grec, _ = E.edge_records(x.astype(np.float64), y.astype(np.float64), E.grid_inflation(x, y, boxes))
    _, out, in_rect = _kept(grec, x, y, rng, 60, 0.6)
    by_rect, by_edges = int(in_rect.sum()), int((in_rect & ~out).sum())
    print(f"  grid, blob(65): the rectangles keep {by_rect}, the edges {by_edges} ({by_edges / by_rect:.3f})")
    assert by_rect > 1000 and by_edges <= 0.75 * by_rect


# ---------------------------------------------------------------------------------------------------------------- GPU: the records
@pytest.mark.gpu
@pytest.mark.parametrize("name", RECORD_CASES)
def test_list_records_on_the_device(hip, name):
    c = LX.CASES[name]
    ref, jx, jy, bounded, twin, info = _twin_of_list_case(name)
    LX.built(c.tris, c.lights, xf=c.ops)(hip)
    hip.render(c.cam, c.w, c.h, c.jitter.shape[0], c.jitter)
    L, R = hip.block_lists(), hip.edge_records()["lists"]
    assert L["leaf"] >= 0 and R.shape[0] == L["entries"].shape[0] > 0
    face = hip.mesh_trees()["tri_src"][L["entries"]["orig"]].astype(np.int64)
    assert E.is_sentinel(R[~bounded[face]]).all(), "an unbounded triangle carries edges"
    ok = bounded[face] & ~ref.near[face]
    live = E.assert_records_hold(R[ok], jx[face][ok], jy[face][ok], name)
    n_rule = E.assert_sentinels_by_rule(R[ok], twin[face][ok], {k: v[face][ok] for k, v in info.items()}, name)
    print(f"\n  {name}: {R.shape[0]} entries, {live} with edges, {int((~bounded[face]).sum())} unbounded, {n_rule} sentinels by the rule")
    if name in ("blob(65)-out", "xf-mirror", "fov-150", "jitter-3.5"):
        assert live > 0.5 * ok.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob(65)", "blob(1025)", "degenerate", "flat-off-plane", "geometric", "blob(65)-mirror", "spanning"])
def test_grid_records_on_the_device(hip, name):
    ST.build(hip, ST.CASES[name])
    pairs, nodes, tris, _ = light_space(hip)
    G = hip.edge_records()["grid"]
    assert G.shape[0] == tris.shape[0]
    seen = np.zeros(G.shape[0], dtype=bool)
    live = grids = 0
    for k in range(pairs.shape[0]):
        idx, x, y, boxes = E.grid_entries(pairs, nodes, tris, k)
        if idx.size == 0:
            continue
        grids += 1
        seen[idx] = True
        live += E.assert_records_hold(G[idx], x, y, f"{name} pair {k}")
        twin, info = E.edge_records(x.astype(np.float64), y.astype(np.float64), E.grid_inflation(x, y, boxes))
        E.assert_sentinels_by_rule(G[idx], twin, info, f"{name} pair {k}")
    assert grids > 0 and E.is_sentinel(G[~seen]).all(), "a record no grid entry points at is not the sentinel"
    print(f"\n  {name}: {grids} grids, {int(seen.sum())} entries, {live} with edges")
    if name in ("blob(65)", "blob(1025)", "blob(65)-mirror"):
        assert live > 0.5 * seen.sum()


# ---------------------------------------------------------------------------------------------------------------- GPU: bit for bit
def off_and_on(ctx, render, what):
    """render() with "edge_cull" 0 and 1: frames and every counter equal.  Returns the frame."""
    out = []
    try:
        for opt in (0, 1):
            ctx.set_option("edge_cull", opt)
            img, st = render()
            out.append((img, counters(st)))
    finally:
        ctx.set_option("edge_cull", 1)
    (a, sa), (b, sb) = out
    assert np.array_equal(a, b), f"{what}: frames differ on {np.count_nonzero(np.any(a != b, axis=-1))} pixels"
    assert sa == sb, what
    return a, sa


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in LX.NAMES if n != "pool"])
def test_list_catalogue_bit_for_bit(hip, name):
    c = LX.CASES[name]
    LX.built(c.tris, c.lights, xf=c.ops)(hip)
    frame, st = off_and_on(hip, lambda: hip.render(c.cam, c.w, c.h, c.jitter.shape[0], c.jitter), name)
    if name in RECORD_CASES:
        H.assert_frames_match(frame, LX.oracle_frame(name), what=name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ST.CASES))
def test_shadow_catalogue_bit_for_bit(hip, name):
    case = ST.CASES[name]
    view = ST.view_of(case)
    ST.build(hip, case)
    jit = ST.jitter(4)
    frame, st = off_and_on(hip, lambda: hip.render(W.camera(view), view.w, view.h, 4, jit, tiles=view.tiles), name)
    assert st["rays_shadow"] > 0
    if name in ("blob(65)", "degenerate", "blob(65)-mirror") and view.tiles is None:
        H.assert_frames_match(frame, ST.reference_frame(name, 4), what=name)


def lower_bunny(ctx, lights):
    ctx.clear()
    mesh = ctx.bsp_mesh(0, TRIS)
    ctx.set_objects(ctx.group([ctx.material(ctx.transform(bunny_ops(), mesh), colour=(0.8, 0.7, 0.6))]))
    for v in lights:
        ctx.add_directional(v, (1, 1, 1))
    ctx.commit()
    return mesh


BW, BH, BSPP = 192, 128, 4
BJIT = ft.jitter_pattern(BSPP)


@pytest.mark.gpu
@pytest.mark.parametrize("lights", [THREE_LIGHTS[:1], THREE_LIGHTS], ids=["one-light", "three-lights"])
@pytest.mark.parametrize("opts", [{}, {"primary_mesh_kernel": 0}, {"primary_block_lists": 0}, {"light_space_shadows": 1}, {"primary_mesh_kernel": 0, "light_space_shadows": 1}],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_bunny_bit_for_bit_under_the_options(hip, lights, opts):
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        lower_bunny(hip, lights)
        before = hip.primary_kernels()
        frame, st = off_and_on(hip, lambda: hip.render(CAM_A, BW, BH, BSPP, BJIT), str(opts))
        after = hip.primary_kernels()
        assert (after["k_primary_mesh"] > before["k_primary_mesh"]) is (opts.get("primary_mesh_kernel", 1) == 1)
        assert st["hits_primary"] > 0 and st["rays_shadow"] > 0
        if not opts:
            orc = O.Oracle()
            lower_bunny(orc, lights)
            H.assert_frames_match(frame, orc.render(CAM_A, BW, BH, BSPP, BJIT)[0], what="bunny")
            orc.close()
    finally:
        hip.set_option("primary_mesh_kernel", 1)
        hip.set_option("primary_block_lists", 1)
        hip.set_option("light_space_shadows", 2)


@pytest.mark.gpu
def test_queued_frames_that_reuse_a_slots_lists(hip):
    """Ten queued frames of one view: from the fifth on a frame reads the lists and the edge records its slot kept; the option flips
    between them, so records written under 0 are read under 1."""
    lower_bunny(hip, THREE_LIGHTS[:2])
    want, _ = hip.render(CAM_B, BW, BH, BSPP, BJIT)
    outs = [ft.PinnedArray((BH, BW, 3)) for _ in range(10)] if hasattr(ft, "PinnedArray") else None
    before = hip.classify_reuse()
    try:
        frames = []
        for k in range(10):
            hip.set_option("edge_cull", 0 if k in (0, 1, 2, 3, 6) else 1)
            if outs:
                hip.render_enqueue(CAM_B, BW, BH, BSPP, BJIT, out=outs[k].array)
            else:
                frames.append(hip.render(CAM_B, BW, BH, BSPP, BJIT)[0])
        if outs:
            hip.wait()
            frames = [o.array for o in outs]
    finally:
        hip.set_option("edge_cull", 1)
    assert hip.classify_reuse()["reused"] > before["reused"]
    for k, f in enumerate(frames):
        assert np.array_equal(np.asarray(f).reshape(want.shape), want), f"queued frame {k}"


@pytest.mark.gpu
def test_after_commit_lights_and_commit_deformed(hip):
    mesh = lower_bunny(hip, THREE_LIGHTS[:2])
    render = lambda: hip.render(CAM_A, BW, BH, BSPP, BJIT)
    off_and_on(hip, render, "committed")
    g0 = hip.edge_records()["grid"].copy()
    hip.set_directional(0, (1.0, -2.0, 0.5), (1, 1, 1))
    hip.commit_lights()
    frame, st = off_and_on(hip, render, "after commit_lights")
    pairs, nodes, tris, _ = light_space(hip)
    G = hip.edge_records()["grid"]
    assert G.shape[0] == tris.shape[0] and (G.shape != g0.shape or not np.array_equal(G, g0)), "the records were not rebuilt with the grid"
    live = 0
    for k in range(pairs.shape[0]):
        idx, x, y, boxes = E.grid_entries(pairs, nodes, tris, k)
        if idx.size:
            live += E.assert_records_hold(G[idx], x, y, f"rebuilt pair {k}")
    assert live > 0
    orc = O.Oracle()
    lower_bunny(orc, [(1.0, -2.0, 0.5), THREE_LIGHTS[1]])
    H.assert_frames_match(frame, orc.render(CAM_A, BW, BH, BSPP, BJIT)[0], what="after commit_lights")
    orc.close()
    # a deformed mesh: its leaf is stripped of its pairs and its shadow rays walk the BVH; the lists are built from the new records
    t = TRIS.copy().reshape(-1, 3, 3)
    t[:, :, 1] *= 1.0 + 0.2 * np.sin(3.0 * t[:, :, 0])
    hip.set_mesh_triangles(mesh, t.reshape(-1, 9))
    hip.commit_deformed()
    off_and_on(hip, render, "after commit_deformed")
    R = hip.edge_records()["lists"]
    assert R.shape[0] == hip.block_lists()["entries"].shape[0] > 0 and not E.is_sentinel(R).all()


@pytest.mark.gpu
def test_through_a_two_device_context(hip):
    lower_bunny(hip, THREE_LIGHTS)
    want, sw = hip.render(CAM_A, BW, BH, BSPP, BJIT)
    two = ft.Context(device=[0, 0])
    try:
        lower_bunny(two, THREE_LIGHTS)
        frame, st = off_and_on(two, lambda: two.render(CAM_A, BW, BH, BSPP, BJIT), "two devices")
        assert np.array_equal(frame, want)
        two.set_directional(1, (1.0, -2.0, 0.5), (1, 1, 1))
        two.commit_lights()
        off_and_on(two, lambda: two.render(CAM_A, BW, BH, BSPP, BJIT), "two devices after commit_lights")
    finally:
        two.close()

"""Option "light_space_retree" (include/functracer_hip.h "moving lights"): ft_scene_commit_lights and
ft_scene_commit_deformed build the topology of the light-space trees they would refit again on the device.

The CPU half checks the option and the header, that a host-only context gives the bytes it gives without the option, the host's topology
generator against the numpy restatement of tests/retree_tools.py word for word, the walk's stack over it, and - on the CPU alone - what a
retree is worth after a quarter turn of the light by a 2-D surface-area cost.

The GPU half walks the light sequences of tests/light_tools.py with the option on and compares, at every step, frames and counters with a
context built from scratch and every retreed pair's child words, leaf-record order and box floats with the numpy replay, bit for bit;
then revisited directions, the way back to the commit's direction, deformations between retrees, the option switched off again, queued
frames, reused classifications, the temporal accumulation, two devices and a mesh large enough for the radix sort's multi-block route.

The byte cap (kLsMaxBytes, 256 MiB) is not reached on the device here: a scene that reaches it takes far longer than a test may.  The
layout arithmetic under a lowered cap is proved in tools/retree_host_check.cpp instead."""
import math
import os

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd._capi import FtError

from . import helpers as H
from . import light_tools as L
from . import retree_tools as R
from . import shadow_tools as S
from . import walk_tools as W
from . import test_temporal as T
from . import test_deform_light_space as D
from .test_light_space_grid import check_grid, grid_of
from .test_light_space_shadows import NONE, check_tree, light_space, pair_root
from .test_mesh_refit import DEFORMS

gpu = pytest.mark.gpu
TOPOLOGY_SIZES = (8, 9, 15, 16, 17, 64, 65, 255, 256, 257, 980, 4097)
WALK_STACK_BOUND = 27                                               # 9 wide levels x 3 pushes, of ls_tree_walk's 64 entries
LSS1_NAMES = ("blob(65)-xf", "chain(256)", "multi-leaf")


# =============================================================================================================================
# CPU half

def test_the_option_exists_and_the_header_names_it():
    ctx = ft.Context(host_only=True)
    for v in (1, 0, 7, -3, 0):
        ctx.set_option("light_space_retree", v)
    with pytest.raises(FtError) as e:
        ctx.set_option("light_space_retrees", 1)
    assert "unknown option" in str(e.value)
    ctx.close()
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    comment = hdr[:hdr.index("int32_t ft_set_option(")]
    assert '"light_space_retree" (0 = default; any other value means 1' in comment[comment.rindex("/*"):]
    paragraph = hdr[:hdr.index("int32_t ft_scene_set_directional(")]
    paragraph = paragraph[paragraph.rindex("/*"):]
    assert '"light_space_retree" 1' in paragraph and "does NOT get that commit's record and grid back" in paragraph
    lib = ft.hip_lib()
    for name in ("ft_debug_ls_retree", "ft_debug_ls_topology"):
        assert f"int32_t {name}(" in hdr and hasattr(lib, name)
    assert lib.ft_abi_version() == 2 and "#define FT_ABI_VERSION 2" in hdr


def _host_state(ctx):
    return [a.tobytes() for a in light_space(ctx)] + [sorted(ctx.scene_info().items())]


def test_host_only_commits_under_the_option_give_the_bytes_they_give_without_it():
    for name in ("multi-leaf", "blob(65)-xf"):
        case = S.CASES[name]
        steps = L.sequence(name)
        on, off = ft.Context(host_only=True), ft.Context(host_only=True)
        on.set_option("light_space_retree", 1)
        on.set_option("deform_light_space", 1)
        handles = {c: D.build(c, case, steps[0][1]) for c in (on, off)}
        for what, lights in steps[1:4]:
            for c in (on, off):
                L.set_lights(c, lights)
                c.commit_lights()
            assert _host_state(on) == _host_state(off), (name, what)
        for how in ("jitter", "twist"):
            for c in (on, off):
                D.deform_to(c, handles[c], D.new_vertices(name, how))
            assert _host_state(on) == _host_state(off), (name, how)
        with pytest.raises(FtError):                               # (no device: no table)
            on.ls_retree()
        on.close()
        off.close()


@pytest.mark.parametrize("n", TOPOLOGY_SIZES)
def test_the_host_generator_is_the_numpy_generator_word_for_word(n):
    for ls_first, first_node in ((0, 0), (1234, 77)):
        child, order, levels = ft.ls_topology(n, ls_first, first_node)
        want_child, want_order, want_levels = R.topology(n, ls_first, first_node)
        assert np.array_equal(child, want_child) and np.array_equal(order, want_order) and np.array_equal(levels, want_levels), (n, ls_first)
        assert len(child) == R.node_count(n)
        # every position in exactly one leaf of 2 .. 4; levels partition the nodes
        leaves = child[(child < 0) & (child != R.EMPTY)]
        first, count = (~leaves) >> 3, (~leaves) & 7
        assert count.min() >= 2 and count.max() <= 4
        covered = np.sort(np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)]))
        assert np.array_equal(covered, np.arange(ls_first, ls_first + n))
        assert sorted(order.tolist()) == list(range(first_node, first_node + len(child))) and int(levels[:, 1].sum()) == len(child)
    for bad in (0, 4):
        with pytest.raises(FtError):
            ft.ls_topology(bad, 0, 0)


def _fake_rec(root):
    rec = np.zeros(16)
    rec[14:15].view(np.int32)[0] = root
    return rec


@pytest.mark.parametrize("n", TOPOLOGY_SIZES + (1 << 20,))
def test_the_walk_holds_at_most_27_pending_entries(n):
    first_node = 5
    child, order, levels = ft.ls_topology(n, 3, first_node)
    assert len(child) == R.node_count(n) and len(levels) <= 9
    assert S.worst_stack(_fake_rec(first_node), R.as_nodes(child, first_node)) <= WALK_STACK_BOUND


# ---- the cost after a quarter turn, on the CPU alone ----------------------------------------------------------------------------------
# refit / retree as measured (DESIGN.md 17.1 has the table).  ASSERTED: exactly the cases at 1.5 and above.  LISTED: the others, with
# their ratios, not asserted - small symmetric blobs and flat or nearly flat sheets have nothing to lose by a turn, and the surface-area
# tree they keep is better than a median tree over a Morton order (whose cost is 1.9 - 2.5 x a fresh surface-area tree's on these cases).
HEIGHT_FIELD = "height-field(32)"
HEIGHT_FIELD_LIGHT, HEIGHT_FIELD_RELIEF = (1.0, -1.0, 0.0), 16.0    # 45 degrees above the field, in the x-y plane; relief of half the side:
# the relief shears the projection by half the field's width along x before the turn and along z after it
ASSERTED = {("flat-in-plane", 0, 1): 1.772, ("multi-leaf", 3, 2): 1.731, (HEIGHT_FIELD, 0, 0): 2.240}
LISTED = {("blob(8)", 0, 0): 0.575, ("blob(8)", 0, 1): 0.421, ("blob(65)-xf", 0, 0): 1.210, ("blob(65)-xf", 0, 1): 0.243,
          ("blob(65)-mirror", 0, 0): 1.017, ("blob(65)-mirror", 0, 1): 0.243, ("concentric", 0, 0): 1.074, ("concentric", 0, 1): 1.046,
          ("flat-in-plane", 0, 0): 0.441, ("two_clusters", 0, 0): 0.467, ("two_clusters", 0, 1): 0.239, ("identical", 0, 0): 1.000,
          ("identical", 0, 1): 1.000, ("chain(256)", 0, 0): 1.437, ("chain(256)", 0, 1): 0.068, ("multi-leaf", 0, 2): 0.575,
          ("multi-leaf", 0, 3): 0.419, ("multi-leaf", 3, 3): 1.401}


def quarter_turn(v):
    """v turned by 90 degrees about the vertical."""
    return (float(v[2]), float(v[1]), float(-v[0]))


def _bare(ctx, tris, v):
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.material(ctx.bsp_mesh(0, np.ascontiguousarray(tris.reshape(-1, 9))), colour=S.MESH_COLOUR)]))
    ctx.add_directional(v, (1, 1, 1))
    ctx.commit()


def _costs(list_recs, old, new, index):
    """(refit, retree): the cost of the old commit's topology boxed again in numpy under the new commit's frame, and of the replayed
    retree under the same frame.  None where either commit gave the pair no tree."""
    pairs, nodes, ls_tris, _ = old
    rec = new[0][index]
    root = pair_root(pairs[index])
    if root < 0 or pair_root(rec) < 0:
        return None
    frame, extent = R.frame_of(rec), R.extent(list_recs, rec[9:12])
    child = nodes[:, 20:24].view(np.int32)
    refit = R.cost(child, R.boxes(child, 0, R.levels_of(child, 0, root), ls_tris, 0, frame, R.pad_of(extent)), 0, root)
    _, new_child, _, _, bx = R.replay(list_recs, 0, 0, 0, rec, extent)
    return refit, R.cost(new_child, bx, 0, 0)


def _quarter_turn_ratios():
    out = {}
    for name in L.NAMES:
        case = S.CASES[name]
        lights = L.initial(case)
        turned = [(l[0], quarter_turn(l[1])) + tuple(l[2:]) if l[0] == "dir" else l for l in lights]
        a, b = ft.Context(host_only=True), ft.Context(host_only=True)
        L.build(a, case, lights)
        L.build(b, case, turned)
        old, new = light_space(a), light_space(b)
        for part, (mesh, _, _) in enumerate(case.parts):
            base = int(old[3][part])
            if base == 0xFFFFFFFF:
                continue
            for l, light in enumerate(lights):
                got = _costs(R.records(S.mesh_tris(mesh)), old, new, base + l) if light[0] == "dir" else None
                if got:
                    out[(name, part, l)] = got
        a.close()
        b.close()
    field = R.height_field(32, HEIGHT_FIELD_RELIEF)
    assert len(field) == 2048
    a, b = ft.Context(host_only=True), ft.Context(host_only=True)
    _bare(a, field, HEIGHT_FIELD_LIGHT)
    _bare(b, field, quarter_turn(HEIGHT_FIELD_LIGHT))
    old, new = light_space(a), light_space(b)
    out[(HEIGHT_FIELD, 0, 0)] = _costs(R.records(field), old, new, int(old[3][0]))
    a.close()
    b.close()
    return out


def test_the_cost_after_a_quarter_turn():
    got = _quarter_turn_ratios()
    for key, (refit, retree) in sorted(got.items()):
        print(f"{key}: refit {refit:.4g} retree {retree:.4g} ratio {refit / retree:.3f}")
    assert set(got) == set(ASSERTED) | set(LISTED)
    assert (HEIGHT_FIELD, 0, 0) in ASSERTED
    assert {k for k, (a, b) in got.items() if a / b >= 1.5} == set(ASSERTED), "the cases at 1.5 and above are not the ones listed as such"
    for key in ASSERTED:
        refit, retree = got[key]
        assert retree < refit, key


# =============================================================================================================================
# GPU half

@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    c.set_option("light_space_retree", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    c = ft.Context(device=0)
    yield c
    c.close()


def _options(ctx, fresh, lss=2, retree=1, deform=0):
    for c in (ctx, fresh):
        c.set_option("light_space_shadows", lss)
    ctx.set_option("light_space_retree", retree)
    ctx.set_option("deform_light_space", deform)


def _render(c, view, spp, **kw):
    return c.render(W.camera(view), view.w, view.h, spp, S.jitter(spp), tiles=view.tiles, **kw)


def _same(ctx, fresh, view, spp, what, shadows=True):
    a, sa = _render(ctx, view, spp)
    b, sb = _render(fresh, view, spp)
    diff = np.any(a != b, axis=2) & ~(np.isnan(a).all(axis=2) & np.isnan(b).all(axis=2))
    assert not diff.any(), f"{what} x{spp}: {int(diff.sum())} pixels differ from the fresh context, first {np.argwhere(diff)[:3].tolist()}"
    assert L.counters(sa) == L.counters(sb), f"{what} x{spp}"
    assert not shadows or sa["rays_shadow"] > 0, what
    return a


def _arrays(ctx):
    return [a.tobytes() for a in light_space(ctx)[:3]]


def check_replay(ctx, recs_of_leaf, what, expect=None):
    """Every pair ls_retree() reports retreed and whose record has a tree now: root, child words, the order of the leaf records and the
    box floats are the numpy replay's, bit for bit, and R is numpy's.  recs_of_leaf(leaf) = the mesh's list-order records.  Returns the
    number of pairs checked."""
    pairs, nodes, ls_tris, _ = light_space(ctx)
    rows = ctx.ls_retree()
    checked = 0
    for row in rows:
        label = f"{what} pair record {row['rec']}"
        if row["block"] >= 0:
            assert row["block_nodes"] == R.node_count(row["n_tris"]) and row["block"] + row["block_nodes"] <= len(nodes), label
        if not row["retreed"]:
            continue
        rec = pairs[row["rec"]]
        if pair_root(rec) == NONE:                                  # unusable now: not retreed in this call
            continue
        assert pair_root(rec) == row["block"], f"{label}: a retreed pair's root is not its block's first node"
        list_recs = recs_of_leaf(row["leaf"])
        n, first, block = row["n_tris"], row["ls_first"], row["block"]
        assert len(list_recs) == n, label
        want_R = R.extent(list_recs, rec[9:12])
        assert abs(row["R"] - want_R) <= 1e-12 * want_R, f"{label}: R {row['R']!r}, numpy {want_R!r}"
        perm, child, order, levels, bx = R.replay(list_recs, 0, first, block, rec, row["R"])
        got = nodes[block:block + len(child)]
        assert np.array_equal(got[:, 20:24].view(np.int32), child), f"{label}: child words"
        assert ls_tris[first:first + n].tobytes() == np.ascontiguousarray(list_recs[perm]).tobytes(), f"{label}: the order of the leaf records"
        assert got[:, :20].tobytes() == bx.reshape(len(child), 20).tobytes(), f"{label}: box floats"
        checked += 1
    if expect is not None:
        assert checked >= expect, f"{what}: {checked} retreed pairs checked, at least {expect} expected"
    return checked


def _case_records(case, tris_of=None):
    tris_of = tris_of or {}

    def recs(leaf):
        mesh = case.parts[leaf][0]
        return R.records(tris_of.get(mesh, S.mesh_tris(mesh)))
    return recs


def _queries_and_planes(ctx, fresh, view, lights, label):
    o, d, _, _ = W.pixel_rays(view)
    ha, hb = ctx.closest(o, d), fresh.closest(o, d)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ha, hb)), label
    v = np.asarray(next(l[1] for l in lights if l[0] == "dir"), dtype=np.float64)
    hit = ha[0].astype(bool)
    origin = (ha[2] + S.SLIGHT_OFFSET * ha[3])[hit]
    back = np.broadcast_to(-v, origin.shape).copy()
    far = np.full(len(origin), 1e300)
    assert np.array_equal(ctx.blocked(origin, back, far), fresh.blocked(origin, back, far)), label
    ga = ctx.render_aov(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
    gb = fresh.render_aov(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
    planes = [key for key in gb if isinstance(gb[key], np.ndarray)]
    assert len(planes) >= 8 and all(ga[key].tobytes() == gb[key].tobytes() for key in planes), label


@gpu
@pytest.mark.parametrize("name,lss", [(n, 2) for n in L.NAMES] + [(n, 1) for n in LSS1_NAMES])
def test_sequence_matches_a_fresh_context_and_the_replay_at_every_step(ctx, fresh, name, lss):
    _options(ctx, fresh, lss=lss)
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps = L.sequence(name)
    L.build(ctx, case, steps[0][1])
    full_nodes = len(light_space(ctx)[1])
    probe = len(steps) // 2
    kept, retreed_ever = {}, 0
    for k, (what, lights) in enumerate(steps[1:], 1):
        L.set_lights(ctx, lights)
        ctx.commit_lights()
        L.build(fresh, case, lights)
        label = f"{name} option {lss} step {k} ({what})"
        _same(ctx, fresh, view, 1, label)
        _same(ctx, fresh, view, 4, label)
        kinds, arrays = L.check_structures(ctx, case, lights, grids=lss == 2)
        assert lss == 2 or all(nu == 0 for nu, _ in kinds.values()), label
        retreed_ever = max(retreed_ever, check_replay(ctx, _case_records(case), label))
        pairs, nodes, _, _ = arrays
        fpairs = light_space(fresh)[0]
        assert pairs[:, :14].tobytes() == fpairs[:, :14].tobytes(), f"{label}: pair doubles [0..13] are not the fresh commit's"
        for row in ctx.ls_retree():
            if row["retreed"] and pair_root(pairs[row["rec"]]) >= 0:
                # the way back too: a retreed pair never takes the full commit's tree or grid again
                assert pair_root(pairs[row["rec"]]) >= full_nodes, label
                at, _, nu, _ = grid_of(pairs[row["rec"]])
                assert nu == 0 or at >= full_nodes * R.NODE_WORDS, f"{label}: a retreed pair's grid lies in the full commit's arrays"
        if what in ("tilted further", "original again"):
            kept[what] = [a.tobytes() for a in arrays[:3]]
        if k == probe:
            _queries_and_planes(ctx, fresh, view, lights, label)
    assert retreed_ever >= 1, f"{name}: no pair was ever retreed"
    rows = ctx.ls_retree()
    assert all(r["retreed"] for r in rows if r["block"] >= 0), f"{name}: {rows}"
    # A, B, A, B, A: the bytes and the sizes of another visit are those of the first
    a_lights, b_lights = steps[3][1], steps[0][1]
    for turn in range(2):
        L.set_lights(ctx, a_lights)
        ctx.commit_lights()
        assert _arrays(ctx) == kept["tilted further"], f"{name}: visit {turn + 2} of the tilted lights left other bytes"
        L.set_lights(ctx, b_lights)
        ctx.commit_lights()
        assert _arrays(ctx) == kept["original again"], f"{name}: visit {turn + 2} of the original lights left other bytes"


@gpu
@pytest.mark.parametrize("name", ("blob(65)-mirror", "multi-leaf"))
def test_two_contexts_through_the_same_sequence_hold_the_same_bytes(ctx, name):
    other = ft.Context(device=0)
    try:
        other.set_option("light_space_retree", 1)
        ctx.set_option("light_space_shadows", 2)
        ctx.set_option("light_space_retree", 1)
        case = S.CASES[name]
        steps = L.sequence(name)
        for c in (ctx, other):
            L.build(c, case, steps[0][1])
        for what, lights in steps[1:]:
            for c in (ctx, other):
                L.set_lights(c, lights)
                c.commit_lights()
            assert [a.tobytes() for a in light_space(ctx)] == [a.tobytes() for a in light_space(other)], (name, what)
    finally:
        other.close()


@gpu
@pytest.mark.parametrize("how", DEFORMS)
@pytest.mark.parametrize("name", ("blob(65)-xf", "multi-leaf"))
def test_deform_retree_deform(ctx, fresh, name, how):
    """Deform, a turned light retrees, deform again: the second gather copies the records in the sorted order, and the deformed commit
    itself retrees the pairs of the meshes it edits."""
    _options(ctx, fresh, deform=1)
    try:
        case, view = S.CASES[name], S.view_of(S.CASES[name])
        base = L.initial(case)
        tilted = [("dir", L.tilt(l[1], math.radians(15.0))) + tuple(l[2:]) if l[0] == "dir" else l for l in base]
        half, whole = D.new_vertices(name, how, 0.5), D.new_vertices(name, how, 1.0)
        handles = D.build(ctx, case, base)
        tris_now, lights_now = {}, base
        for what, tris_of, lights in (("deformed half way", half, base), ("the lights tilted", half, tilted), ("deformed all the way", whole, tilted)):
            if tris_of is not tris_now and tris_of:
                D.deform_to(ctx, handles, tris_of)
            if lights is not lights_now:
                L.set_lights(ctx, lights)
                ctx.commit_lights()
            tris_now, lights_now = tris_of, lights
            label = f"{name} {how}: {what}"
            D.build(fresh, case, lights, tris_of)
            D.same_structures(ctx, fresh, case, lights, tris_of, label)      # the leaf records as a multiset, check_tree, the grids' cells
            D.same_frames(ctx, fresh, view, label)
            check_replay(ctx, _case_records(case, {m: t.reshape(-1, 3, 3) for m, t in tris_of.items()}), label, expect=1)
    finally:
        ctx.set_option("deform_light_space", 0)


@gpu
def test_option_0_after_1_refits_over_the_new_topology(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps = L.sequence(name)
    L.build(ctx, case, steps[0][1])
    L.set_lights(ctx, steps[3][1])
    ctx.commit_lights()
    assert check_replay(ctx, _case_records(case), "retreed") == 2
    after_retree = light_space(ctx)
    ctx.set_option("light_space_retree", 0)
    try:
        for what, lights in (steps[5], steps[0], steps[3]):
            L.set_lights(ctx, lights)
            ctx.commit_lights()
            L.build(fresh, case, lights)
            label = f"option 0 after 1: {what}"
            _same(ctx, fresh, view, 1, label)
            _same(ctx, fresh, view, 4, label)
            L.check_structures(ctx, case, lights)
            rows = ctx.ls_retree()
            assert all(r["retreed"] for r in rows), label
            pairs, nodes, ls_tris, _ = light_space(ctx)
            for r in rows:                                          # still the block's tree over the records as the retree ordered them
                assert pair_root(pairs[r["rec"]]) == r["block"], label
                span = slice(r["ls_first"], r["ls_first"] + r["n_tris"])
                assert ls_tris[span].tobytes() == after_retree[2][span].tobytes(), label
                block = slice(r["block"], r["block"] + r["block_nodes"])
                assert nodes[block, 20:24].tobytes() == after_retree[1][block, 20:24].tobytes(), label
    finally:
        ctx.set_option("light_space_retree", 1)


@gpu
def test_a_pair_unusable_at_the_zero_direction_is_retreed_once_it_is_usable_again(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-mirror"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps = dict(L.sequence(name))
    L.build(ctx, case, L.sequence(name)[0][1])
    L.set_lights(ctx, steps["zero"])
    ctx.commit_lights()                                             # the only light that changes has no usable frame: nothing is retreed
    rows = ctx.ls_retree()
    assert len(rows) == 2 and not any(r["retreed"] for r in rows), rows
    L.build(fresh, case, steps["zero"])
    _same(ctx, fresh, view, 1, "zero")
    L.check_structures(ctx, case, steps["zero"])
    L.set_lights(ctx, steps["usable again"])
    ctx.commit_lights()
    assert sorted(r["retreed"] for r in ctx.ls_retree()) == [False, True]      # the other light never turned
    L.build(fresh, case, steps["usable again"])
    _same(ctx, fresh, view, 1, "usable again")
    _same(ctx, fresh, view, 4, "usable again")
    L.check_structures(ctx, case, steps["usable again"])
    assert check_replay(ctx, _case_records(case), "usable again") == 1


@gpu
def test_a_frame_queued_before_the_call_shows_the_old_lights(ctx, fresh):
    _options(ctx, fresh)
    case, view = S.CASES["blob(65)-xf"], S.view_of(S.CASES["blob(65)-xf"])
    steps = L.sequence("blob(65)-xf")
    L.build(ctx, case, steps[0][1])
    old, _ = _render(ctx, view, 1)
    ctx.render_enqueue(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
    L.set_lights(ctx, steps[3][1])
    ctx.commit_lights()                                             # retires the queued frame first
    assert np.array_equal(ctx.fetch_frame(np.zeros((view.h, view.w, 3))), old)
    L.build(fresh, case, steps[3][1])
    new = _same(ctx, fresh, view, 1, "after a queued frame")
    assert not np.array_equal(new, old)
    assert check_replay(ctx, _case_records(case), "after a queued frame") == 2


@gpu
def test_a_reused_classification_does_not_outlive_the_call(ctx, fresh):
    _options(ctx, fresh)
    case, view = S.CASES["concentric"], S.view_of(S.CASES["concentric"])
    steps = L.sequence("concentric")
    L.build(ctx, case, steps[0][1])
    first, _ = _render(ctx, view, 1)
    again, _ = _render(ctx, view, 1)                                # the same view twice: the slot's classification is reused
    assert np.array_equal(first, again)
    L.set_lights(ctx, steps[3][1])
    ctx.commit_lights()
    L.build(fresh, case, steps[3][1])
    _same(ctx, fresh, view, 1, "after a reused classification")
    _same(ctx, fresh, view, 4, "after a reused classification")


@gpu
def test_the_temporal_accumulation_stays_open(ctx, fresh):
    """Two accumulates, a commit_lights that retrees, a third: the history continues and the set is test_temporal's restatement's."""
    _options(ctx, fresh)
    case, view = S.CASES["blob(65)-xf"], S.view_of(S.CASES["blob(65)-xf"])
    steps = L.sequence("blob(65)-xf")
    L.build(ctx, case, steps[0][1])
    cam, w, h, jit = W.camera(view), view.w, view.h, S.jitter(1)
    inside = np.ones((h, w), dtype=bool)
    ctx.temporal_begin(w, h)
    st = T.new_state(h, w)
    frames = []
    for k in range(3):
        if k == 2:
            L.set_lights(ctx, steps[3][1])
            ctx.commit_lights()
            assert any(r["retreed"] for r in ctx.ls_retree())
        c, _ = ctx.render(cam, w, h, 1, jit, seed=100 + k)
        frames.append(c)
        p, n, leaf = T._surfaces(ctx, cam, w, h, 1, jit, 0, 100 + k)
        ctx.temporal_accumulate(cam, 1, jit, sample=0, seed=100 + k)
        st = T.reference(st, T.image_plane(cam, w, h), c, p, n, leaf, inside)
        T._compare(ctx, st, inside & ~st["taint"], f"retree call {k}")
        status = ctx.temporal_status()
        assert status["calls"] == k + 1
    assert not np.array_equal(frames[2], frames[1])
    assert status["with_history"] > 0 and status["with_history"] >= int(st["history"].sum()) - int(st["taint"].sum())
    ctx.temporal_end()


def _two_devices(two, fresh):
    ordinals = two.devices()
    try:
        two.set_option("light_space_retree", 1)
        fresh.set_option("light_space_shadows", 2)
        name = "multi-leaf"
        case, view = S.CASES[name], S.view_of(S.CASES[name])
        steps = L.sequence(name)
        L.build(two, case, steps[0][1])
        for k, (what, lights) in enumerate(steps[1:], 1):
            L.set_lights(two, lights)
            two.commit_lights()
            L.build(fresh, case, lights)
            for spp in (1, 4):
                a, sa = _render(two, view, spp)
                b, _ = _render(fresh, view, spp)
                assert np.array_equal(a, b, equal_nan=True), f"{ordinals} step {k} ({what}) x{spp}"
                assert sa["rays_shadow"] > 0
            L.check_structures(two, case, lights)
            check_replay(two, _case_records(case), f"{ordinals} step {k}")
        assert any(r["retreed"] for r in two.ls_retree())
    finally:
        two.close()


@gpu
def test_two_devices(fresh):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _two_devices(ft.Context(device=[0, 1]), fresh)


@gpu
def test_two_device_context_on_one_gpu(fresh):
    _two_devices(ft.Context(device=[0, 0]), fresh)


@gpu
def test_a_mesh_past_the_sorts_single_block_route(ctx, fresh):
    """91 x 91 quads, 16 562 triangles: structure, replay and one frame against a fresh context."""
    _options(ctx, fresh)
    field = R.height_field(91, 6.0)
    assert len(field) >= 16384
    tris = np.ascontiguousarray(field.reshape(-1, 9))
    view = W.View("height-field(91)", np.array([45.0, 120.0, -60.0]), np.array([45.0, 0.0, 45.0]), 50.0, 96, 72, None, None)

    def build(c, v):
        c.clear()
        ground = c.transform([("scale", (400.0, 1.0, 400.0)), ("translate", (-150.0, -20.0, -150.0))], c.primitive(ft.SQUARE))
        c.set_objects(c.group([c.material(c.bsp_mesh(0, tris), colour=S.MESH_COLOUR), c.material(ground, colour=S.RECEIVER_COLOUR)]))
        c.add_directional(v, (1, 1, 1))
        c.commit()

    first, turned = (1.0, -2.0, 1.0), (-1.5, -1.0, 0.4)
    build(ctx, first)
    ctx.set_directional(0, turned, (1, 1, 1))
    ctx.commit_lights()
    build(fresh, turned)
    _same(ctx, fresh, view, 1, "height-field(91)")
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    rec = pairs[int(leaf_pairs[0])]
    assert check_tree(rec, nodes, ls_tris) == len(field)
    if grid_of(rec)[2] > 0:
        check_grid(rec, nodes, ls_tris, len(field))
    assert S.worst_stack(rec, nodes) <= WALK_STACK_BOUND
    assert check_replay(ctx, lambda leaf: R.records(field), "height-field(91)") == 1

"""Option "moved_in_place" (include/functracer_hip.h "moving rigid objects"): ft_scene_commit_moved uploads the new poses
over the old ones and brings the light-space shadow structures up to them on the device instead of committing the scene again, through
the pose sequences of tests/move_tools.py.

The CPU half checks the new entry point, that a host-only context accepts the option and still takes the full host commit (byte for
byte a fresh context's, counted with reason 1), and on the oracle alone that every step of every sequence changes the frame and keeps a
shadow in view - but for the step that makes the only caster of a one-caster case singular, where nothing is left to cast one.

The GPU half walks every sequence with one in-place commit_moved per step and compares frame, counters, surface buffers and leaf
matrices with a second context built from scratch at that pose, bit for bit; then what a call leaves in device memory (the mesh trees
untouched, the pair records a fresh commit's, the trees and grids sound, the first commit's bytes back at the original pose), the hazard
of a light or a deformation after a move, every fallback with its reason code, the orderings, the temporal accumulation and a
two-device context."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import helpers as H
from . import light_tools as L
from . import move_tools as MV
from . import shadow_tools as S
from . import walk_tools as W
from . import test_temporal_motion as M
from .test_light_space_grid import grid_of
from .test_light_space_shadows import NONE, light_space, pair_root

gpu = pytest.mark.gpu
ALL = MV.NAMES + (MV.HAND,)
MIN_SHADOW = 20


def test_header_declares_and_library_exports_the_call():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    lib = ft.hip_lib()
    assert "int32_t ft_debug_moved_commits(ft_context* ctx, int64_t out[4]);" in hdr and hasattr(lib, "ft_debug_moved_commits")
    assert '"moved_in_place"' in hdr
    assert lib.ft_abi_version() == 2 and "#define FT_ABI_VERSION 2" in hdr
    assert callable(ft.Context.moved_commits)
    ctx = ft.Context(host_only=True)
    out = (C.c_int64 * 4)()
    assert lib.ft_debug_moved_commits(None, out) == -1 and lib.ft_debug_moved_commits(ctx._ctx, None) == -1
    assert ctx.moved_commits() == {"in_place": 0, "full": 0, "full_reason": 0, "pairs_refit": 0}
    ctx.close()


def test_axis_is_parallel_to_no_light():
    axis = np.asarray(MV.AXIS) / np.linalg.norm(MV.AXIS)
    for name in MV.NAMES:
        for l in S.CASES[name].lights:
            if l[0] != "point":
                v = np.asarray(l[1], dtype=np.float64)
                assert abs(float(axis @ v) / float(np.linalg.norm(v))) < 0.95, (name, l)
    assert abs(float(axis @ np.array([0.4, -1.0, 0.6])) / math.sqrt(0.16 + 1.0 + 0.36)) < 0.95   # the hand scene's


def _state(ctx):
    return [a.tobytes() for a in ctx.leaf_matrices()] + [a.tobytes() for a in light_space(ctx)] + [sorted(ctx.scene_info().items())]


@pytest.mark.parametrize("name", ALL)
def test_host_only_accepts_the_option_and_takes_the_full_commit(name):
    ctx = ft.Context(host_only=True)
    ctx.set_option("moved_in_place", 1)                             # (an unknown option before it existed)
    ctx.set_option("moved_in_place", 7)                             # any other value means 1
    steps = MV.steps_of(name)
    hd = MV.build_any(ctx, name, steps[0][2])
    for k, (_, what, pose) in enumerate(steps[1:], 1):
        MV.move(ctx, hd, pose)
        fresh = ft.Context(host_only=True)
        MV.build_any(fresh, name, pose)
        assert _state(ctx) == _state(fresh), (name, what)
        fresh.close()
        assert ctx.moved_commits() == {"in_place": 0, "full": k, "full_reason": _capi.MOVED_OPTION_OFF, "pairs_refit": 0}
    ctx.close()


@pytest.mark.parametrize("name", ALL)
def test_every_step_changes_the_frame_and_keeps_a_shadow_on_the_oracle(name):
    """A condition on the reference alone, so that the device comparisons are not vacuous: consecutive steps' frames differ, and on the
    shadow cases at least 20 receiver pixels in view lie in some directional light's shadow at every step - except where a case's only
    caster stands under the singular scale: a ray taken into its model space is not finite and hits nothing, so there is no caster."""
    steps = MV.steps_of(name)
    if name == MV.HAND:
        frames, counts = MV.oracle_hand_frames(), None
    else:
        seen = MV.oracle_steps(name)
        frames, counts = [f for _, f in seen], [n for n, _ in seen]
        print(f"{name}: receiver pixels shadowed per step {[(what, n) for (_, what, _), n in zip(steps, counts)]}")
    for k, (kind, what, _) in enumerate(steps):
        if counts is not None and not (kind == MV.SINGULAR and len(S.CASES[name].parts) == 1):
            assert counts[k] >= MIN_SHADOW, (name, what, counts[k])
        if k:
            assert not np.array_equal(frames[k], frames[k - 1]), (name, what)


# =============================================================================================================================
# GPU half

@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    c.set_option("moved_in_place", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    c = ft.Context(device=0)
    yield c
    c.close()


def _options(contexts, shadows=2, retree=0, **more):
    for c in contexts:
        c.set_option("light_space_shadows", shadows)
        c.set_option("light_space_retree", retree)
        for k, v in more.items():
            c.set_option(k, v)


def _same(ctx, fresh, name, what, spp=MV.SPP):
    a, sa = MV.render(ctx, name, spp)
    b, sb = MV.render(fresh, name, spp)
    diff = np.any(a != b, axis=2) & ~(np.isnan(a).all(axis=2) & np.isnan(b).all(axis=2))
    assert not diff.any(), f"{what} x{spp}: {int(diff.sum())} pixels differ from the fresh context, first {np.argwhere(diff)[:3].tolist()}"
    assert L.counters(sa) == L.counters(sb), f"{what} x{spp}"
    assert sa["rays_shadow"] > 0, what
    return a


def _same_surfaces(ctx, fresh, name, what):
    ga, gb = MV.render_aov(ctx, name), MV.render_aov(fresh, name)
    planes = [key for key in gb if isinstance(gb[key], np.ndarray)]
    assert len(planes) >= 8 and all(ga[key].tobytes() == gb[key].tobytes() for key in planes), what
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ctx.leaf_matrices(), fresh.leaf_matrices())), what


def _in_place(ctx, before, what):
    now = ctx.moved_commits()
    assert now["in_place"] == before["in_place"] + 1 and now["full"] == before["full"] and now["full_reason"] == _capi.MOVED_NOT_FULL, (what, before, now)
    return now


@gpu
@pytest.mark.parametrize("retree", (0, 1))
@pytest.mark.parametrize("shadows", (0, 1, 2))
@pytest.mark.parametrize("name", ALL)
def test_every_step_in_place_matches_a_fresh_context(ctx, fresh, name, shadows, retree):
    _options((ctx, fresh), shadows, retree)
    steps = MV.steps_of(name)
    hd = MV.build_any(ctx, name, steps[0][2])
    previous = None
    for k, (kind, what, pose) in enumerate(steps[1:], 1):
        before = ctx.moved_commits()
        MV.move(ctx, hd, pose)
        label = f"{name} shadows {shadows} retree {retree} step {k} ({what})"
        now = _in_place(ctx, before, label)
        times = ctx.commit_times()
        print(f"{label}: pairs refit {now['pairs_refit']}, host {times['flatten_ms']:.3f} ms, kernels {times['device_bvh_ms']:.3f} ms, uploads {times['upload_ms']:.3f} ms")
        MV.build_any(fresh, name, pose)
        frame = _same(ctx, fresh, name, label)
        _same_surfaces(ctx, fresh, name, label)
        assert previous is None or not np.array_equal(frame, previous), f"{label}: the frame did not change"
        previous = frame
        if shadows == 0:
            assert now["pairs_refit"] == 0 and times["device_bvh_ms"] == 0.0, label
        elif kind == MV.TURN:
            assert now["pairs_refit"] > 0 and times["device_bvh_ms"] > 0.0, label
    _options((ctx, fresh))


def _translated(pose, keys, by):
    out = {k: list(v) for k, v in pose.items()}
    for k in keys:
        out[k] = out[k] + [("translate", by)]
    return out


@gpu
@pytest.mark.parametrize("name", ALL)
def test_a_translation_launches_no_kernel(ctx, fresh, name):
    """From the committed pose and from a turned one: no pair's frame changes, so ft_get_commit_times[1] is exactly 0 and no pair is refit."""
    _options((ctx, fresh))
    steps = MV.steps_of(name)
    keys = ("sphere", "mesh", "cube") if name == MV.HAND else MV.MOVERS[name] + ("receiver",)
    turned = steps[3][2]                                            # 30 degrees
    assert steps[3][0] == MV.TURN and steps[1][0] == MV.TRANSLATE
    hd = MV.build_any(ctx, name, steps[0][2])
    for what, pose, translation in (("slid", steps[1][2], True), ("turned", turned, False), ("turned and slid", _translated(turned, keys, (0.07, -0.02, 0.05)), True),
                                    ("slid further", _translated(turned, keys, (0.11, 0.03, -0.04)), True)):
        before = ctx.moved_commits()
        MV.move(ctx, hd, pose)
        now = _in_place(ctx, before, f"{name} {what}")
        kernels = ctx.commit_times()["device_bvh_ms"]
        if translation:
            assert kernels == 0.0 and now["pairs_refit"] == 0, (name, what, kernels, now)
        else:
            assert kernels > 0.0 and now["pairs_refit"] > 0, (name, what, kernels, now)
        MV.build_any(fresh, name, pose)
        _same(ctx, fresh, name, f"{name} {what}")


TREE_ARRAYS = ("nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes")


@gpu
@pytest.mark.parametrize("name", ("multi-leaf", MV.HAND))
def test_no_mesh_tree_is_rebuilt_or_moved(ctx, name):
    """"bvh_builder" 3: the device builds the tree of every mesh, whatever its size.  What ft_debug_mesh_trees reads back from device memory
    is the same before and after every in-place step, byte for byte."""
    _options((ctx,), bvh_builder=3)
    try:
        steps = MV.steps_of(name)
        hd = MV.build_any(ctx, name, steps[0][2])
        first = ctx.mesh_trees()
        assert first["from_device"] and first["jobs"]
        for k, (_, what, pose) in enumerate(steps[1:], 1):
            before = ctx.moved_commits()
            MV.move(ctx, hd, pose)
            _in_place(ctx, before, f"{name} step {k}")
            now = ctx.mesh_trees()
            assert all(now[key].tobytes() == first[key].tobytes() for key in TREE_ARRAYS) and now["jobs"] == first["jobs"] and now["stack_capacity"] == first["stack_capacity"], (name, what)
    finally:
        _options((ctx,), bvh_builder=2)


def _moved_records(pairs, leaf_pairs, case, parts):
    """{(part, light): record} of the directional lights' pairs of the given casters."""
    out = {}
    for part in parts:
        base = int(leaf_pairs[part])
        assert base != 0xFFFFFFFF
        for l, _ in S.dir_lights(case):
            out[(part, l)] = pairs[base + l]
    return out


@gpu
@pytest.mark.parametrize("retree", (0, 1))
@pytest.mark.parametrize("shadows", (1, 2))
@pytest.mark.parametrize("name", MV.NAMES)
def test_structures_in_device_memory_after_each_step(ctx, fresh, name, shadows, retree):
    """After every step the moved pairs' record doubles [0..13] are a fresh commit's (a pair without a usable frame has root INT32_MIN in
    both), and light_tools.check_structures passes on what ft_debug_light_space reads back: every triangle in conservative boxes on its
    path, every grid the one build_grid's rule picks, listing every triangle in every cell its box overlaps; the walk's stack bound holds.
    Back at the original pose the pair records are the first commit's and so are the arrays, byte for byte and at the same sizes - unless
    the pairs were retreed ("light_space_retree" 1), which have no way back to that commit's tree: their records' doubles [0..13] are that
    commit's, their root is their block's."""
    _options((ctx, fresh), shadows, retree)
    case = S.CASES[name]
    lights = L.initial(case)
    steps = MV.sequence(name)
    movers = MV.MOVERS[name]
    hd = MV.build(ctx, case, steps[0][2])
    first = light_space(ctx)
    first_recs = _moved_records(first[0], first[3], case, movers)
    for k, (kind, what, pose) in enumerate(steps[1:], 1):
        MV.move(ctx, hd, pose)
        MV.build(fresh, case, pose)
        label = f"{name} shadows {shadows} retree {retree} step {k} ({what})"
        pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
        want = light_space(fresh)
        got_recs = _moved_records(pairs, leaf_pairs, case, movers)
        singular = kind == MV.SINGULAR
        for key, rec in got_recs.items():
            if singular and key[0] == movers[0]:                    # (a fresh commit gives a leaf none of whose pairs has a tree no records at all)
                assert pair_root(rec) == NONE and grid_of(rec)[2] == 0, (label, key)
                assert int(want[3][key[0]]) == 0xFFFFFFFF or pair_root(want[0][int(want[3][key[0]]) + key[1]]) == NONE, (label, key)
                continue
            want_rec = _moved_records(want[0], want[3], case, (key[0],))[key]
            assert rec[:14].tobytes() == want_rec[:14].tobytes(), (label, key)
            assert pair_root(rec) >= 0 and S.worst_stack(rec, nodes) <= S.WAVE_STACK, (label, key)
        if not singular:
            kinds, _ = L.check_structures(ctx, case, lights, grids=shadows == 2)
            assert shadows == 2 or all(nu == 0 for nu, _ in kinds.values()), label
            if shadows == 2 and name != "two_clusters" and kind == MV.TURN:
                assert any(nu > 0 for (part, _), (nu, _) in kinds.items() if part in movers), (label, kinds)   # a grid was built on the device
    # the last step is the original pose
    assert steps[-1][0] == MV.ORIGINAL
    rows = ctx.ls_retree()
    moved_rows = [r for r in rows if any(r["rec"] == int(first[3][part]) + l for part in movers for l, _ in S.dir_lights(case))]
    assert len(moved_rows) == len(first_recs)
    if retree:
        assert all(r["retreed"] for r in moved_rows), rows
        for key, rec in got_recs.items():
            assert rec[:14].tobytes() == first_recs[key][:14].tobytes() and pair_root(rec) != pair_root(first_recs[key]), key
    else:
        assert not any(r["retreed"] for r in rows)
        for key, rec in got_recs.items():
            assert rec.tobytes() == first_recs[key].tobytes(), key
        for a, b, which in zip((pairs, nodes, ls_tris), first, ("pair records", "nodes", "triangle records")):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name} shadows {shadows}: the {which} are not the first commit's"
    _options((ctx, fresh))


@gpu
@pytest.mark.parametrize("shadows", (1, 2))
def test_a_light_back_at_its_first_direction_over_a_turned_leaf(ctx, fresh, shadows):
    """The hazard: a caster turned in place, its light turned with commit_lights and then turned back to the full commit's direction.
    That commit's record and grid describe another orientation of the leaf: the pair must not get them back."""
    _options((ctx, fresh), shadows)
    name = "blob(65)-mirror"
    case = S.CASES[name]
    steps, lights = MV.sequence(name), L.sequence(name)
    turned = steps[3][2]
    hd = MV.build(ctx, case, steps[0][2])
    first = light_space(ctx)
    first_recs = _moved_records(first[0], first[3], case, (0,))
    MV.move(ctx, hd, turned)
    for what, ls in (("turned in place", lights[0][1]), ("the lights tilted", lights[3][1]), ("the lights back", lights[0][1]), ("the lights exchanged", lights[1][1]),
                     ("the lights back again", lights[0][1])):
        if what != "turned in place":
            L.set_lights(ctx, ls)
            ctx.commit_lights()
        MV.build(fresh, case, turned, lights=ls)
        _same(ctx, fresh, name, f"shadows {shadows}: {what}")
        pairs, _, _, leaf_pairs = light_space(ctx)
        want = light_space(fresh)
        for key, rec in _moved_records(pairs, leaf_pairs, case, (0,)).items():
            assert rec[:14].tobytes() == _moved_records(want[0], want[3], case, (0,))[key][:14].tobytes(), (what, key)
            assert rec[:14].tobytes() != first_recs[key][:14].tobytes(), (what, key)
        L.check_structures(ctx, case, ls, grids=shadows == 2)
    # and the way back still exists: the leaf at the full commit's pose again under that commit's lights
    MV.move(ctx, hd, steps[0][2])
    MV.build(fresh, case, steps[0][2])
    _same(ctx, fresh, name, "back at the original pose")
    got = light_space(ctx)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], first[:3]))
    _options((ctx, fresh))


@gpu
def test_a_deformed_commit_after_a_move_in_place(ctx, fresh):
    """The same question asked by ft_scene_commit_deformed under "deform_light_space": one caster turned in place, then ANOTHER mesh
    deformed.  The deformed commit lays the region behind the full commit's arrays out anew; the turned caster's pairs are not the full
    commit's, although their light still points where it did, and must be laid out with it."""
    _options((ctx, fresh), 2, 0, deform_light_space=1)
    try:
        name = "multi-leaf"
        case = S.CASES[name]
        steps = MV.sequence(name)
        only_big = {k: list(v) for k, v in steps[0][2].items()}
        only_big[3] = steps[3][2][3]                                # the 65-triangle caster turned by 30 degrees, the 8-triangle one where it was
        hd = MV.build(ctx, case, steps[0][2])
        first = light_space(ctx)
        MV.move(ctx, hd, only_big)
        assert ctx.moved_commits()["full_reason"] == _capi.MOVED_NOT_FULL
        tris = S.mesh_tris(case.parts[0][0]).reshape(-1, 9)
        for what, bent in (("bent", tris * np.array([1.0, 1.05, 0.97] * 3)), ("bent further", tris * np.array([1.1, 0.9, 1.0] * 3)), ("straight again", tris * 1.0)):
            ctx.set_mesh_triangles(hd["meshes"][0], bent)
            ctx.commit_deformed()
            MV.build(fresh, case, only_big, tris={0: bent})
            _same(ctx, fresh, name, f"deformed after a move: {what}")
            pairs, _, _, leaf_pairs = light_space(ctx)
            want = light_space(fresh)
            for key, rec in _moved_records(pairs, leaf_pairs, case, (3,)).items():
                assert rec[:14].tobytes() == _moved_records(want[0], want[3], case, (3,))[key][:14].tobytes(), (what, key)
                assert rec[:14].tobytes() != _moved_records(first[0], first[3], case, (3,))[key][:14].tobytes(), (what, key)
            L.check_structures(ctx, case, L.initial(case))
        # a move in place after the deformation: the deformed pairs stay deformed, the turned ones come back
        before = ctx.moved_commits()
        MV.move(ctx, hd, steps[0][2])
        _in_place(ctx, before, "back after the deformation")
        MV.build(fresh, case, steps[0][2], tris={0: tris * 1.0})
        _same(ctx, fresh, name, "back after the deformation")
        L.check_structures(ctx, case, L.initial(case))
    finally:
        _options((ctx, fresh), deform_light_space=0)


def _full(ctx, before, reason, what):
    now = ctx.moved_commits()
    assert now["full"] == before["full"] + 1 and now["in_place"] == before["in_place"] and now["full_reason"] == reason and now["pairs_refit"] == 0, (what, before, now)


@gpu
def test_pending_edits_take_the_full_commit(ctx, fresh):
    """A pending light setter, pending vertices and a pending commit-time option have always been absorbed by the full commit a moved
    commit was: they still are, with reason 2, and the bits are a fresh context's."""
    _options((ctx, fresh))
    name = "two_clusters"
    case = S.CASES[name]
    steps, lights = MV.sequence(name), L.sequence(name)
    hd = MV.build(ctx, case, steps[0][2])
    tris = S.mesh_tris(case.parts[0][0]).reshape(-1, 9)
    # a light setter
    before = ctx.moved_commits()
    L.set_lights(ctx, lights[3][1])
    MV.move(ctx, hd, steps[3][2])
    _full(ctx, before, _capi.MOVED_PENDING, "a pending light setter")
    MV.build(fresh, case, steps[3][2], lights=lights[3][1])
    _same(ctx, fresh, name, "a pending light setter")
    # new vertices
    before = ctx.moved_commits()
    bent = tris * np.array([1.0, 1.04, 1.0] * 3)
    ctx.set_mesh_triangles(hd["meshes"][0], bent)
    MV.move(ctx, hd, steps[4][2])
    _full(ctx, before, _capi.MOVED_PENDING, "pending vertices")
    MV.build(fresh, case, steps[4][2], lights=lights[3][1], tris={0: bent})
    _same(ctx, fresh, name, "pending vertices")
    # a commit-time option
    before = ctx.moved_commits()
    ctx.set_option("light_space_shadows", 1)
    fresh.set_option("light_space_shadows", 1)
    MV.move(ctx, hd, steps[5][2])
    _full(ctx, before, _capi.MOVED_PENDING, "a pending commit-time option")
    MV.build(fresh, case, steps[5][2], lights=lights[3][1], tris={0: bent})
    _same(ctx, fresh, name, "a pending commit-time option")
    assert all(grid_of(rec)[2] == 0 for rec in light_space(ctx)[0])
    # nothing pending any more: in place again
    before = ctx.moved_commits()
    MV.move(ctx, hd, steps[6][2])
    _in_place(ctx, before, "nothing pending")
    MV.build(fresh, case, steps[6][2], lights=lights[3][1], tris={0: bent})
    _same(ctx, fresh, name, "nothing pending")
    # the option off: reason 1
    before = ctx.moved_commits()
    ctx.set_option("moved_in_place", 0)
    MV.move(ctx, hd, steps[2][2])
    _full(ctx, before, _capi.MOVED_OPTION_OFF, "the option off")
    ctx.set_option("moved_in_place", 1)
    _options((ctx, fresh))


def _same_union(ctx, fresh, what):
    cam, w, h = MV.union_camera(), MV.UNION_CAM["w"], MV.UNION_CAM["h"]
    for spp in (1, MV.SPP):
        a, sa = ctx.render(cam, w, h, spp, S.jitter(spp))
        b, sb = fresh.render(cam, w, h, spp, S.jitter(spp))
        assert np.array_equal(a, b, equal_nan=True) and L.counters(sa) == L.counters(sb), f"{what} x{spp}"
    o = np.broadcast_to(np.asarray(MV.UNION_CAM["o"], dtype=np.float64), (64, 3)).copy()
    d = np.stack([np.array([-1.5 + 0.05 * k, -2.0 + 0.01 * k, 5.0]) for k in range(64)])
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ctx.closest(o, d), fresh.closest(o, d))), what
    assert sorted(ctx.scene_info().items()) == sorted(fresh.scene_info().items()), what
    return a


@gpu
def test_an_item_that_crosses_six_face_directions_takes_the_full_commit(ctx, fresh):
    """A union of three cubes: five face directions while C stands along the axes, seven once it turns about x - more than a cull record
    holds, so the item's OP_CULL pair leaves the program: reason 3, both ways."""
    _options((ctx, fresh))
    hd = MV.build_union(ctx, MV.union_pose())
    assert ctx.scene_info()["face_directions"] == 5
    words = ctx.scene_info()["program_words"]
    previous = None
    for what, pose, in_place in (("slid", MV.union_pose(whole=(0.5, 1.0, 0.0)), True), ("B turned further", MV.union_pose(b_deg=50.0, whole=(0.5, 1.0, 0.0)), True),
                                 ("the union turned", MV.union_pose(b_deg=50.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), True),
                                 ("C turned: past six", MV.union_pose(b_deg=50.0, c_deg=20.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), False),
                                 ("C turned further", MV.union_pose(b_deg=50.0, c_deg=35.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), True),
                                 ("C back: five again", MV.union_pose(b_deg=50.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), False), ("original", MV.union_pose(), True)):
        before = ctx.moved_commits()
        MV.move(ctx, hd, pose)
        if in_place:
            _in_place(ctx, before, what)
        else:
            _full(ctx, before, _capi.MOVED_DIFFERS, what)
        MV.build_union(fresh, pose)
        frame = _same_union(ctx, fresh, what)
        assert previous is None or not np.array_equal(frame, previous), what
        previous = frame
        assert (ctx.scene_info()["program_words"] == words) == ("C turned" not in what), what


def _many_directions(tilt_deg):
    """Ten cubes turned about ten different axes (30 face directions), a tilted square (1) and a square that lies flat (the receiver's
    direction) or, tilted, brings one more."""
    cubes = [[("scale", 0.3), ("rotate", (1.0 + 0.3 * k, 2.0 - 0.1 * k, 0.5 + 0.2 * k), 0.3 + 0.17 * k), ("translate", (-2.0 + 0.45 * k, 0.4, 1.5))] for k in range(10)]
    flat = ([("rotate", (1.0, 0.0, 0.2), math.radians(tilt_deg))] if tilt_deg else []) + [("translate", (0.8, 0.6, -0.8))]
    return cubes, [("rotate", (0.3, 0.0, 1.0), 0.4), ("translate", (-1.2, 0.5, -0.6))], flat


def _build_many(b, tilt_deg, flat=None):
    cubes, tilted, flat_of_tilt = _many_directions(tilt_deg)
    flat = flat_of_tilt if flat is None else flat
    b.clear()
    items = [b.material(b.transform([("scale", (8.0, 1.0, 8.0)), ("translate", (-4.0, 0.0, -4.0))], b.primitive(ft.SQUARE)), colour=(0.6, 0.6, 0.6))]
    for ops in cubes:
        items.append(b.material(b.transform(ops, b.primitive(ft.CUBE)), colour=(0.3, 0.5, 0.8)))
    items.append(b.material(b.transform(tilted, b.primitive(ft.SQUARE)), colour=(0.8, 0.5, 0.3)))
    hd = {"flat": b.transform(flat, b.primitive(ft.SQUARE))}
    items.append(b.material(hd["flat"], colour=(0.4, 0.8, 0.4)))
    b.set_objects(b.group(items))
    b.add_directional((0.3, -1.0, 0.2), (1.0, 1.0, 1.0))
    b.commit()
    return hd


@gpu
def test_from_32_to_33_face_directions(ctx, fresh):
    """The scene-wide table holds 32 directions; a square that tilts brings the 33rd and the wave-level pre-test goes off for the whole
    scene (face_directions -1).  Whichever way the call takes, the bits are a fresh context's.  (It takes the full commit: the table's
    length is a launch argument and sizes an array)"""
    _options((ctx, fresh))
    hd = _build_many(ctx, 0.0)
    assert ctx.scene_info()["face_directions"] == 32
    for what, tilt, directions in (("slid only", None, 32), ("tilted", 15.0, -1), ("tilted further", 25.0, -1), ("flat again", 0.0, 32)):
        before = ctx.moved_commits()
        flat = _many_directions(tilt or 0.0)[2] + ([("translate", (0.1, 0.0, 0.1))] if tilt is None else [])
        ctx.set_transform(hd["flat"], flat)
        ctx.commit_moved()
        now = ctx.moved_commits()
        assert now["in_place"] + now["full"] == before["in_place"] + before["full"] + 1
        print(f"32 -> 33 face directions, {what}: {'in place' if now['full_reason'] == 0 else 'full commit, reason %d' % now['full_reason']}")
        _build_many(fresh, tilt or 0.0, flat=flat)
        _same_union(ctx, fresh, what)
        assert ctx.scene_info()["face_directions"] == directions, what


@gpu
def test_ordering_with_queued_frames_reuse_and_the_progressive_accumulation(ctx, fresh):
    _options((ctx, fresh))
    name = "blob(65)-mirror"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps = MV.sequence(name)
    hd = MV.build(ctx, case, steps[0][2])
    cam, jit = W.camera(view), S.jitter(1)
    # a frame queued before the call shows the old pose and arrives whole
    old, _ = MV.render(ctx, name, 1)
    ctx.render_enqueue(cam, view.w, view.h, 1, jit, tiles=view.tiles)
    before = ctx.moved_commits()
    MV.move(ctx, hd, steps[3][2])                                   # retires the queued frame first
    _in_place(ctx, before, "after a queued frame")
    assert np.array_equal(ctx.fetch_frame(np.zeros((view.h, view.w, 3))), old)
    MV.build(fresh, case, steps[3][2])
    new = _same(ctx, fresh, name, "after a queued frame", spp=1)
    assert not np.array_equal(new, old)
    # a kept classification does not outlive the call
    again, _ = MV.render(ctx, name, 1)
    assert np.array_equal(again, new)
    slots = 4                                                       # a context's frame slots are taken in turn: each keeps its own classification
    for _ in range(slots):
        MV.render(ctx, name, 1)
    reuse = ctx.classify_reuse()
    for _ in range(slots):
        MV.render(ctx, name, 1)
    after = ctx.classify_reuse()
    assert after["reused"] == reuse["reused"] + slots and after["classified"] == reuse["classified"], (reuse, after)   # the same view again: reused
    reuse = after
    MV.move(ctx, hd, steps[1][2])                                   # a translation: no kernel, still another scene
    for _ in range(slots):
        MV.render(ctx, name, 1)
    after = ctx.classify_reuse()
    assert after["reused"] == reuse["reused"] and after["classified"] == reuse["classified"] + slots, (reuse, after)
    MV.build(fresh, case, steps[1][2])
    _same(ctx, fresh, name, "after a reused classification", spp=1)
    _same(ctx, fresh, name, "after a reused classification")
    # a progressive accumulation ends
    ctx.progressive_begin(cam, view.w, view.h)
    ctx.progressive_pass(2, ft.jitter_pattern(2), seed=1, fetch=False)
    MV.move(ctx, hd, steps[4][2])
    jit2 = ft.jitter_pattern(2)
    assert ft.hip_lib().ft_progressive_pass(ctx._ctx, 2, _capi.dptr(jit2), 2, 0, None, None) == -5
    ctx._progressive = None


@gpu
@pytest.mark.parametrize("which", ("sliding sphere", "mixed"))
def test_temporal_accumulation_is_the_same_in_place(which):
    """The 6-call sequences of tests/test_temporal_motion.py, once with the option 0 and once with 1, device against device: M, Q, N and
    ft_temporal_status bitwise equal, the accumulation open throughout."""
    cam, jit = M._camera(), np.zeros((1, 2))
    pose = (lambda k: M._pose(float(k), sphere_only=True, sphere_step=0.4)) if which == "sliding sphere" else (lambda k: M._pose(float(k)))
    runs = []
    for option in (0, 1):
        c = ft.Context(device=0)
        try:
            c.set_option("moved_in_place", option)
            hd = M._build(c, pose(0))
            c.temporal_begin(M.W, M.Hh)
            for k in range(M.CALLS):
                if k:
                    M._move(c, hd, pose(k))
                    assert c.temporal_status()["calls"] == k       # still open
                c.render(cam, M.W, M.Hh, 1, jit, seed=700 + k, fetch=False)
                c.temporal_accumulate(cam, 1, jit, seed=700 + k, fetch=False)
            runs.append(c.temporal_fetch() + (c.temporal_status(),))
            counts = c.moved_commits()
            assert (counts["in_place"], counts["full"]) == ((M.CALLS - 1, 0) if option else (0, M.CALLS - 1)), counts
            c.temporal_end()
        finally:
            c.close()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0][:3], runs[1][:3])) and runs[0][3] == runs[1][3]
    assert runs[0][3]["calls"] == M.CALLS and runs[0][3]["with_history"] > 0


@gpu
def test_two_device_context_on_one_gpu(fresh):
    """A context over devices [0, 0], as test_multi_device_context_equals_single_device builds it: the turning steps of multi-leaf, every
    frame a single-device fresh context's."""
    two = ft.Context(device=[0, 0])
    try:
        two.set_option("moved_in_place", 1)
        _options((two, fresh))
        name = "multi-leaf"
        case = S.CASES[name]
        steps = MV.sequence(name)
        hd = MV.build(two, case, steps[0][2])
        for k, (kind, what, pose) in enumerate(steps[1:7], 1):
            before = two.moved_commits()
            MV.move(two, hd, pose)
            _in_place(two, before, f"[0, 0] step {k}")
            MV.build(fresh, case, pose)
            for spp in (1, MV.SPP):
                a, sa = MV.render(two, name, spp)
                b, _ = MV.render(fresh, name, spp)
                assert np.array_equal(a, b, equal_nan=True), f"[0, 0] step {k} ({what}) x{spp}"
                assert sa["rays_shadow"] > 0
            L.check_structures(two, case, L.initial(case))
    finally:
        two.close()

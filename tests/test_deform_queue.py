"""Queued deform commits (include/functracer_hip.h "queued deform commits"): ft_scene_commit_deformed_enqueue commits new
mesh vertices without retiring a queued frame or waiting for a stream a frame runs on, through the scene and poses of
tests/deform_queue_tools.py.

The CPU half checks the entry points, the twin's FT_ERR_STATE rules in the twin's order, that a host-only context takes the blocking
path with reason 1, and on the oracle alone that consecutive poses differ in at least 1 % of the frame's pixels.

The GPU half: a step is { edit, queued commit, queued frame into its own page-locked buffer }, twelve of them before one wait, and frame
k must be bitwise what a context built from scratch with pose k's vertices renders - so a refit that reached the frames too early or too
late, or a geometry set handed out while a frame still read it, shows as a wrong frame.  Then every kind of edit, two meshes edited in
turn (the carry between sets), the refusals with frames in flight, every fallback with its reason code, the pose queue interleaved,
every blocking call once the live set is no longer the scene's own arrays, what may follow a queued call, the queued temporal calls, and
a context that never uses the feature.  Every comparison is bitwise."""
import ctypes as C
import os

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import bvh_tools as B
from . import deform_queue_tools as D
from . import helpers as H
from . import light_tools as L
from . import test_temporal_queue as TQ
from .test_light_space_shadows import light_space
from .test_mesh_refit import list_range

gpu = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5
ZEROS = dict(zip(_capi.DEFORM_QUEUE_FIELDS, [0] * 8))
BUILDERS = (0, 3)               # the host's trees and the device's: both range layouts are refit


# =============================================================================================================================
# CPU half

def test_header_declares_and_library_exports_the_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    lib = ft.hip_lib()
    for decl, name in (("int32_t ft_scene_commit_deformed_enqueue(ft_context* ctx);", "ft_scene_commit_deformed_enqueue"),
                       ("int32_t ft_debug_deform_queue(ft_context* ctx, int64_t out[8]);", "ft_debug_deform_queue")):
        assert decl in hdr and hasattr(lib, name), name
    assert lib.ft_abi_version() == 2 and "#define FT_ABI_VERSION 2" in hdr      # additions only
    assert all(callable(getattr(ft.Context, k)) for k in ("commit_deformed_enqueue", "deform_queue"))
    assert _capi.GEO_SETS_MAX == D.FRAME_SLOTS + _capi.TEMPORAL_QUEUE_DEPTH + 1 == 9


def test_null_arguments():
    lib = ft.hip_lib()
    out = (C.c_int64 * 8)()
    assert lib.ft_scene_commit_deformed_enqueue(None) == ERR_INVALID
    ctx = ft.Context(host_only=True)
    assert lib.ft_debug_deform_queue(None, out) == ERR_INVALID and lib.ft_debug_deform_queue(ctx._ctx, None) == ERR_INVALID
    assert ctx.deform_queue() == ZEROS
    ctx.close()


def test_state_rules_are_the_twins_in_the_twins_order():
    """Each refusal of ft_scene_commit_deformed is the queued call's: the same code and the same message from the same state, nothing
    counted; with several reasons to refuse, the same one is named."""
    lib = ft.hip_lib()
    base = D.arm()[0]

    def held(c):
        return D.build(c, base, D.plane())

    def pending_transform(c):
        c.set_transform(held(c)["xf"], [("translate", (0.1, 0.0, 0.0))])

    def pending_light(c):
        held(c)
        c.set_positional(1, *D.point_light(1))

    states = {
        "no held commit": lambda c: None,
        "a structural change": lambda c: (held(c), c.primitive(ft.SPHERE)),
        "a pending transform": pending_transform,
        "a commit-time option": lambda c: (held(c), c.set_option("light_space_shadows", 1)),
        "a pending light": pending_light,
        # the order: restructured before moved before options before lights
        "structural + transform": lambda c: (pending_transform(c), c.primitive(ft.SPHERE)),
        "transform + option + light": lambda c: (pending_transform(c), c.set_option("light_space_shadows", 1), c.set_positional(1, *D.point_light(1))),
        "option + light": lambda c: (pending_light(c), c.set_option("light_space_shadows", 1)),
    }
    for what, prepare in states.items():
        seen = []
        for call in (lib.ft_scene_commit_deformed, lib.ft_scene_commit_deformed_enqueue):
            c = ft.Context(host_only=True)
            prepare(c)
            seen.append((call(c._ctx), lib.ft_last_error(c._ctx)))
            assert c.deform_queue() == ZEROS, what
            c.close()
        assert seen[0][0] == seen[1][0] == ERR_STATE and seen[0][1] == seen[1][1], (what, seen)


@pytest.mark.parametrize("kind", ("bones", "weights", "verts"))
def test_host_only_call_takes_the_blocking_path(kind):
    """Byte for byte the blocking twin's scene, counted as a call that took the blocking path with reason 1; no geometry set exists."""
    ctx, twin = ft.Context(host_only=True), ft.Context(host_only=True)
    hd, ht = D.prepare(ctx, kind), D.prepare(twin, kind)
    for k in (1, 2, 3):
        D.edit(ctx, hd, kind, k), D.edit(twin, ht, kind, k)
        ctx.commit_deformed_enqueue()
        twin.commit_deformed()
        a, b = ctx.mesh_trees(), twin.mesh_trees()
        assert all(a[key].tobytes() == b[key].tobytes() for key in ("nodes", "bsp_leaves", "tris", "wide", "coarse_boxes")), (kind, k)
        assert ctx.scene_info() == twin.scene_info(), (kind, k)
        assert ctx.deform_queue() == dict(ZEROS, blocking=k, reason=_capi.DEFORM_HOST_ONLY), (kind, k)
    # a refusal is the twin's too, and is not counted
    bad = D.expected("verts", 1).copy()
    bad[5, 4] = np.nan
    if kind == "verts":
        for c, call in ((ctx, ctx.commit_deformed_enqueue), (twin, twin.commit_deformed)):
            c.set_mesh_triangles(hd["arm"], bad)
            with pytest.raises(ft.FtError) as e:
                call()
            assert e.value.status == ERR_UNSUPPORTED
        assert ctx.deform_queue() == dict(ZEROS, blocking=3, reason=_capi.DEFORM_HOST_ONLY)
    ctx.close(), twin.close()


@pytest.mark.parametrize("kind", ("bones", "weights", "dq", "weights+bones", "two meshes"))
def test_consecutive_poses_differ_on_the_oracle(kind):
    """A condition on the reference alone, so that a stale frame cannot pass: consecutive poses differ in at least 1 % of the frame's
    pixels ("verts" and "host-skin" are "bones"' vertices)."""
    frames = D.oracle_frames("bones", True) if kind == "two meshes" else D.oracle_frames(kind)
    counts = [D.changed(a, b) for a, b in zip(frames, frames[1:])]
    print(f"{kind}: pixels changed per step {counts} of {frames[0].shape[0] * frames[0].shape[1]}")
    assert len(counts) == D.STEPS and min(counts) >= D.MIN_CHANGED_FRACTION * frames[0].shape[0] * frames[0].shape[1], (kind, counts)


# =============================================================================================================================
# GPU half

@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    c = ft.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pinned():
    """Page-locked frames, made once: pinned(shape, n) -> n float64 arrays."""
    made = {}

    def get(shape, n=D.STEPS):
        have = made.setdefault(tuple(shape), [])
        while len(have) < n:
            have.append(ft.PinnedArray(shape, np.float64))
        return [p.array for p in have[:n]]

    yield get
    for ps in made.values():
        for p in ps:
            p.close()


def _options(contexts, builder=0, shadows=2, **more):
    defaults = dict(refit_rebuild_percent=0, deform_light_space=0, temporal_follow_deformed=0, skin_on_device=1, morph_on_device=1, moved_in_place=0)
    for c in contexts:
        c.set_option("bvh_builder", builder)
        c.set_option("light_space_shadows", shadows)
        for k, v in {**defaults, **more}.items():
            c.set_option(k, v)


def _counters(st):
    return {k: v for k, v in L.counters(st).items() if k != "n_launches"}     # (the level hint restarts: n_launches depends on it)


_FRESH = {}


def _fresh(fresh, builder, arm_tris_key, spp, shadows=2, ops=None, point=None, plane_k=0):
    """(frame, counters) of a context built from scratch with the vertices `arm_tris_key` = (kind, k) names: computed once, shared, never
    changed."""
    key = (builder, arm_tris_key, spp, shadows, str(ops), str(point), plane_k)
    if key not in _FRESH:
        _options((fresh,), builder, shadows)
        D.build(fresh, D.expected(*arm_tris_key), D.plane(plane_k), ops=ops, point=point)
        frame, st = fresh.render(*D.frame_args(spp))
        frame.setflags(write=False)
        _FRESH[key] = (frame, _counters(st))
    return _FRESH[key]


def _delta(c, before):
    now = c.deform_queue()
    return {k: now[k] - before[k] if k in ("queued", "blocking", "retired_for_set") else now[k] for k in now}


def _same_frame(got, want, what):
    assert np.array_equal(got, want, equal_nan=True), f"{what}: {D.changed(got, want)} pixels differ"


def _queued(c, hd, kind, k, reason=_capi.DEFORM_QUEUED, what=""):
    before = c.deform_queue()
    D.edit(c, hd, kind, k)
    c.commit_deformed_enqueue()
    d = _delta(c, before)
    assert d["reason"] == reason and (d["queued"], d["blocking"]) == ((1, 0) if reason == _capi.DEFORM_QUEUED else (0, 1)), (what, d)
    return d


# ---------------------------------------------------------------------------------------------------------------- 1. ordering
@gpu
@pytest.mark.parametrize("spp", (4, 16))
@pytest.mark.parametrize("builder", BUILDERS)
def test_twelve_queued_poses_each_frame_a_fresh_contexts(ctx, fresh, pinned, builder, spp):
    """More steps than geometry sets, so sets are reused while frames are in flight; at 160 x 90 x 16 the frames really overlap the refits."""
    _options((ctx,), builder)
    args = D.frame_args(spp)
    bufs = pinned((args[2], args[1], 3))
    hd = D.prepare(ctx, "bones")
    before = ctx.deform_queue()
    for k in range(1, D.STEPS + 1):
        D.edit(ctx, hd, "bones", k)
        ctx.commit_deformed_enqueue()
        bufs[k - 1][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[k - 1])
    counted = _delta(ctx, before)                                   # (the frames are still in flight)
    st = ctx.wait()
    print(f"builder {builder} x{spp}: {counted}")
    for k in range(1, D.STEPS + 1):
        _same_frame(bufs[k - 1], _fresh(fresh, builder, ("bones", k), spp)[0], f"builder {builder} x{spp}: frame {k} is not the fresh context's")
    assert _counters(st) == _fresh(fresh, builder, ("bones", D.STEPS), spp)[1]
    assert counted["queued"] == D.STEPS and counted["blocking"] == 0 and counted["reason"] == _capi.DEFORM_QUEUED, counted
    # the host retired nothing for the commits: when the last one returned, the frames of the steps before it were still pending
    assert counted["pending"] == D.pending_at_last_call(D.STEPS - 1) == D.FRAME_SLOTS, counted
    assert 2 <= counted["sets"] <= _capi.GEO_SETS_MAX, counted
    times = ctx.commit_times()
    assert times["device_bvh_ms"] > 0.0 and times["flatten_ms"] > 0.0 and times["upload_ms"] > 0.0, times   # (a palette: the scan's readback is waited for)
    assert ctx.skin(hd["arm"])["device_meshes"] == 1


# ---------------------------------------------------------------------------------------------------------------- 2. every kind of edit
@gpu
@pytest.mark.parametrize("kind", ("weights", "dq", "weights+bones", "verts", "host-skin"))
@pytest.mark.parametrize("builder", BUILDERS)
def test_every_kind_of_edit_is_queued(ctx, fresh, pinned, builder, kind):
    _options((ctx,), builder)
    args = D.frame_args(4)
    bufs = pinned((args[2], args[1], 3))
    hd = D.prepare(ctx, kind)
    before = ctx.deform_queue()
    for k in range(1, 7):
        _queued(ctx, hd, kind, k, what=kind)
        bufs[k - 1][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[k - 1])
    counted = _delta(ctx, before)
    ctx.wait()
    for k in range(1, 7):
        _same_frame(bufs[k - 1], _fresh(fresh, builder, (kind, k), 4)[0], f"builder {builder}, {kind}: frame {k}")
    assert counted["queued"] == 6 and counted["pending"] == D.FRAME_SLOTS, counted
    times = ctx.commit_times()
    if kind in ("verts", "host-skin"):                              # every vertex came from the host: no kernel of the call is waited for
        assert times["device_bvh_ms"] == 0.0, times
    counts = {"weights": ctx.morph, "dq": ctx.skin_dq, "weights+bones": ctx.skin}.get(kind)
    if counts:
        assert counts(hd["arm"])["device_meshes"] == 1, kind
    if kind == "host-skin":
        assert ctx.skin(hd["arm"])["host_meshes"] == 1 and ctx.skin(hd["arm"])["device_meshes"] == 0
    ctx.set_option("skin_on_device", 1)


# ---------------------------------------------------------------------------------------------------------------- 3. the carry
@gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_two_meshes_edited_in_turn_are_carried_between_sets(ctx, fresh, pinned, builder):
    """The arm is posed on even steps, the plane rippled on odd ones, a frame queued behind each: the set a call picks is behind the live
    one for the mesh it does not edit, and k_refit_carry brings that mesh's ranges over."""
    _options((ctx,), builder)
    args = D.frame_args(4)
    bufs = pinned((args[2], args[1], 3))
    hd = D.prepare(ctx, "bones")
    ctx.set_mesh_triangles(hd["plane"], D.plane(0))
    ctx.commit_deformed()
    carried = []
    for k in range(1, D.STEPS + 1):
        ka, kp = D.two_mesh_state(k)
        if k % 2 == 0:
            D.edit(ctx, hd, "bones", ka)
        else:
            ctx.set_mesh_triangles(hd["plane"], D.plane(kp))
        ctx.commit_deformed_enqueue()
        d = ctx.deform_queue()
        assert d["reason"] == _capi.DEFORM_QUEUED, (k, d)
        carried.append(d["carried"])
        bufs[k - 1][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[k - 1])
    ctx.wait()
    print(f"builder {builder}: ranges carried per step {carried}")
    for k in range(1, D.STEPS + 1):
        ka, kp = D.two_mesh_state(k)
        _same_frame(bufs[k - 1], _fresh(fresh, builder, ("bones", ka), 4, plane_k=kp)[0], f"builder {builder}: frame {k}")
    assert max(carried) > 0, carried
    # The trees as they lie in device memory.  A fresh context BUILDS its trees over the new vertices, so its topology is its own: what
    # it shares with a refit tree, bit for bit, is every list-order record (a record is made from its triangle's vertices alone).  The
    # whole of ft_debug_mesh_trees - topology, boxes, sorted copies, 4-wide nodes, coarse boxes - is compared with a twin that made the
    # same edits through the blocking call, and checked against the structure rules every builder is held to.
    ka, kp = D.two_mesh_state(D.STEPS)
    _options((fresh,), builder)
    D.build(fresh, D.expected("bones", ka), D.plane(kp))
    got, want = ctx.mesh_trees(), fresh.mesh_trees()
    for mesh in (0, 1):
        first, n = list_range(got, mesh)
        assert (first, n) == list_range(want, mesh) and n in (312, 72)
        assert got["tris"][first:first + n].tobytes() == want["tris"][first:first + n].tobytes(), f"builder {builder}: the records of mesh {mesh} are not the fresh context's"
    twin = ft.Context(device=0)
    try:
        _options((twin,), builder)
        ht = D.prepare(twin, "bones")
        for k in range(0, D.STEPS + 1):
            ka, kp = D.two_mesh_state(k)
            if k % 2 == 0:
                D.edit(twin, ht, "bones", ka)
            else:
                twin.set_mesh_triangles(ht["plane"], D.plane(kp))
            twin.commit_deformed()
        want = twin.mesh_trees()
    finally:
        twin.close()
    for key in ("nodes", "bsp_leaves", "tris", "tri_orig", "wide", "coarse_boxes", "meshes"):
        assert got[key].tobytes() == want[key].tobytes(), f"builder {builder}: {key} of ft_debug_mesh_trees is not the blocking twin's"
    B.check_trees(got)


# ---------------------------------------------------------------------------------------------------------------- 4. the old pose in flight
@gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_frame_queued_in_front_of_a_call_shows_the_old_pose(ctx, fresh, pinned, builder):
    _options((ctx,), builder)
    args = D.frame_args(16)
    bufs = pinned((args[2], args[1], 3))
    hd = D.prepare(ctx, "bones")
    for k in range(1, 7):
        bufs[k - 1][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[k - 1])                  # pose k - 1, still running when the call below returns
        d = _queued(ctx, hd, "bones", k)
        assert d["pending"] == min(k, D.FRAME_SLOTS), (k, d)
    ctx.wait()
    for k in range(1, 7):
        _same_frame(bufs[k - 1], _fresh(fresh, builder, ("bones", k - 1), 16)[0], f"builder {builder}: the frame in front of call {k}")


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
SHRUNK = 0.5                    # the refusal scene: the arm's vertices shrunk by this under a transform that scales them back


def _shrunk_palette(k):
    p = D.palette(k).reshape(D.BONES, 3, 4).copy()
    p[:, :, 3] *= SHRUNK                                            # the pivots shrink with the vertices
    return p.reshape(D.BONES, 12)


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_refusals_with_frames_in_flight_leave_the_old_pose(ctx, fresh, pinned, builder):
    """A palette whose products overflow (a non-finite vertex) and one that leaves finite vertices which the leaf's transform takes past
    1e300 (the item loses its bounds): FT_ERR_UNSUPPORTED, nothing counted, and the frame in flight and the next frame are the old pose's.
    The arm stands under a scale of 2 here, its vertices shrunk to match, so that finite vertices can lose their bounds."""
    _options((ctx, fresh), builder)
    args = D.frame_args(4)
    bufs = pinned((args[2], args[1], 3))
    base, index, weight = D.arm()
    ops = [("scale", (1.0 / SHRUNK,) * 3)]
    hd = D.build(ctx, base * SHRUNK, D.plane(), ops=ops)
    ctx.set_mesh_skin(hd["arm"], index, weight)
    ctx.set_mesh_bones(hd["arm"], _shrunk_palette(0))
    ctx.commit_deformed()

    def fresh_frame(k):
        D.build(fresh, ft.skin_blend(base * SHRUNK, index, weight, _shrunk_palette(k)), D.plane(), ops=ops)
        return fresh.render(*args)[0]

    ctx.set_mesh_bones(hd["arm"], _shrunk_palette(1))
    ctx.commit_deformed_enqueue()
    assert ctx.deform_queue()["reason"] == _capi.DEFORM_QUEUED
    want = fresh_frame(1)
    assert D.changed(want, fresh_frame(0)) >= D.MIN_CHANGED_FRACTION * args[1] * args[2]
    overflow = np.full((D.BONES, 12), 1e308)
    huge = np.tile(np.array([5e299, 0, 0, 0, 0, 5e299, 0, 0, 0, 0, 5e299, 0]), (D.BONES, 1))
    with np.errstate(all="ignore"):
        assert not np.isfinite(ft.skin_blend(base * SHRUNK, index, weight, overflow)).all()
        v = ft.skin_blend(base * SHRUNK, index, weight, huge)
        assert np.abs(v).max() < 1e300 and np.abs(v).max() / SHRUNK > 1e300
    before = ctx.deform_queue()
    for n, (bones, why) in enumerate(((overflow, "non-finite"), (huge, "bounds"))):
        bufs[2 * n][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[2 * n])                  # in flight
        ctx.set_mesh_bones(hd["arm"], bones)
        assert ctx._lib.ft_scene_commit_deformed_enqueue(ctx._ctx) == ERR_UNSUPPORTED and why in ctx.last_error(), (why, ctx.last_error())
        d = _delta(ctx, before)
        assert d["queued"] == 0 and d["blocking"] == 0, (why, d)
        bufs[2 * n + 1][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[2 * n + 1])              # the next frame: the old commit is still renderable
        ctx.wait()
        _same_frame(bufs[2 * n], want, f"{why}: the frame in flight")
        _same_frame(bufs[2 * n + 1], want, f"{why}: the next frame")
    ctx.render_enqueue(*args)
    ctx.set_mesh_bones(hd["arm"], _shrunk_palette(3))               # a good pose afterwards works
    ctx.commit_deformed_enqueue()
    assert ctx.deform_queue()["reason"] == _capi.DEFORM_QUEUED and ctx.deform_queue()["pending"] == 1
    _same_frame(ctx.render(*args)[0], fresh_frame(3), "a good pose after the refusals")


# ---------------------------------------------------------------------------------------------------------------- 6. fallbacks
@gpu
@pytest.mark.parametrize("reason", (_capi.DEFORM_FIRST_REFIT, _capi.DEFORM_REBUILD, _capi.DEFORM_LIGHT_SPACE, _capi.DEFORM_TEMPORAL_FOLLOW))
def test_fallbacks_give_the_blocking_twins_bits_and_report_why(reason):
    builder = 3
    more = {_capi.DEFORM_REBUILD: dict(refit_rebuild_percent=100), _capi.DEFORM_LIGHT_SPACE: dict(deform_light_space=1),
            _capi.DEFORM_TEMPORAL_FOLLOW: dict(temporal_follow_deformed=1)}.get(reason, {})
    args = D.frame_args(4)
    cam, w, h, spp, jit = args
    work, twin = ft.Context(device=0), ft.Context(device=0)
    try:
        _options((work, twin), builder, **more)
        base, index, weight = D.arm()
        hds = []
        for c in (work, twin):
            hd = D.build(c, base, D.plane())
            c.set_mesh_skin(hd["arm"], index, weight)
            if reason != _capi.DEFORM_FIRST_REFIT:
                D.edit(c, hd, "bones", 0)
                c.commit_deformed()
            hds.append(hd)
        if reason == _capi.DEFORM_TEMPORAL_FOLLOW:
            for c in (work, twin):
                c.temporal_begin(w, h)
                c.render(*args, fetch=False)
                c.temporal_accumulate(cam, spp, jit, sample=spp - 1, fetch=False)
        for k in (1, 2):
            work.render_enqueue(*args)                              # in flight: the fallback retires it, as the twin does
            _queued(work, hds[0], "bones", k, reason if (k == 1 or reason != _capi.DEFORM_FIRST_REFIT) else _capi.DEFORM_QUEUED, what=f"reason {reason}")
            assert work.deform_queue()["pending"] == (0 if (k == 1 or reason != _capi.DEFORM_FIRST_REFIT) else 1)
            D.edit(twin, hds[1], "bones", k)
            twin.commit_deformed()
            a, b = work.render(*args), twin.render(*args)
            _same_frame(a[0], b[0], f"reason {reason}, pose {k}")
            assert _counters(a[1]) == _counters(b[1])
            if reason == _capi.DEFORM_LIGHT_SPACE:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(light_space(work), light_space(twin))), k
            if reason == _capi.DEFORM_TEMPORAL_FOLLOW:
                outs = [c.temporal_accumulate(cam, spp, jit, sample=spp - 1)[0] for c in (work, twin)]
                _same_frame(outs[0], outs[1], f"the history that follows the triangles, pose {k}")
            ta, tb = work.mesh_trees(), twin.mesh_trees()
            assert all(ta[key].tobytes() == tb[key].tobytes() for key in ("nodes", "tris", "wide", "coarse_boxes")), (reason, k)
    finally:
        work.close(), twin.close()


@gpu
def test_two_device_context_takes_the_blocking_path(fresh):
    two = ft.Context(device=[0, 0])
    try:
        _options((two,))
        args = D.frame_args(4)
        hd = D.prepare(two, "bones")
        for k in (1, 2, 3):
            two.render_enqueue(*args)
            d = _queued(two, hd, "bones", k, _capi.DEFORM_MULTI_DEVICE)
            assert d["pending"] == 0 and d["sets"] == 1, d
            _same_frame(two.render(*args)[0], _fresh(fresh, 0, ("bones", k), 4)[0], f"[0, 0]: pose {k}")
    finally:
        two.close()


# ---------------------------------------------------------------------------------------------------------------- 7. with the pose queue
@gpu
@pytest.mark.parametrize("lights", (False, True))
@pytest.mark.parametrize("shadows", (0, 2))
def test_interleaved_with_queued_pose_and_light_commits(ctx, fresh, pinned, shadows, lights):
    _options((ctx,), 0, shadows)
    args = D.frame_args(4)
    bufs = pinned((args[2], args[1], 3))
    hd = D.prepare(ctx, "bones")
    before, pose_before = ctx.deform_queue(), ctx.pose_queue()
    n = 8
    for k in range(1, n + 1):
        ctx.set_transform(hd["xf"], D.slide(k))
        ctx.commit_moved_enqueue()
        if lights:
            ctx.set_positional(1, *D.point_light(k))
            ctx.commit_lights_enqueue()
        D.edit(ctx, hd, "bones", k)
        ctx.commit_deformed_enqueue()
        bufs[k - 1][...] = 0.0
        ctx.render_enqueue(*args, out=bufs[k - 1])
    counted, pose = _delta(ctx, before), ctx.pose_queue()
    ctx.wait()
    for k in range(1, n + 1):
        want = _fresh(fresh, 0, ("bones", k), 4, shadows, ops=D.slide(k), point=D.point_light(k) if lights else None)[0]
        _same_frame(bufs[k - 1], want, f"shadows {shadows}, lights {lights}: frame {k}")
    assert counted["queued"] == n and counted["blocking"] == 0 and counted["pending"] == D.FRAME_SLOTS, counted
    assert pose["moved_queued"] - pose_before["moved_queued"] == n and pose["moved_blocking"] == pose_before["moved_blocking"], pose
    assert pose["lights_queued"] - pose_before["lights_queued"] == (n if lights else 0), pose


# ---------------------------------------------------------------------------------------------------------------- 8. blocking calls off set 0
def _off_set_zero(c, hd, args, k):
    """A queued call with a frame in flight, so that the live geometry set is not the scene's own arrays; then the frame is retired."""
    c.render_enqueue(*args)
    d = _queued(c, hd, "bones", k)
    assert d["sets"] >= 2 and d["pending"] == 1, d
    c.wait()


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_blocking_calls_with_the_live_set_off_set_zero(ctx, fresh, builder):
    args = D.frame_args(4)
    _options((ctx,), builder)
    hd = D.prepare(ctx, "bones")
    # the blocking twin, plain
    _off_set_zero(ctx, hd, args, 1)
    D.edit(ctx, hd, "bones", 2)
    ctx.commit_deformed()
    _same_frame(ctx.render(*args)[0], _fresh(fresh, builder, ("bones", 2), 4)[0], "commit_deformed")
    # the tree quality, read from the live set: what a context that never queued measures
    _off_set_zero(ctx, hd, args, 3)
    twin = ft.Context(device=0)
    try:
        _options((twin,), builder)
        ht = D.prepare(twin, "bones")
        D.edit(twin, ht, "bones", 3)
        twin.commit_deformed()
        assert ctx.tree_quality(hd["arm"])["cost"] == twin.tree_quality(ht["arm"])["cost"]
        # under "refit_rebuild_percent" (a device-built tree is rebuilt in the live set; queued calls behind it carry the new topology)
        for c in (ctx, twin):
            c.set_option("refit_rebuild_percent", 100)
        _queued(ctx, hd, "bones", 9, _capi.DEFORM_REBUILD)
        D.edit(twin, ht, "bones", 9)
        twin.commit_deformed()
        _same_frame(ctx.render(*args)[0], twin.render(*args)[0], "commit_deformed under refit_rebuild_percent")
        assert ctx.tree_quality(hd["arm"])["rebuilds"] == twin.tree_quality(ht["arm"])["rebuilds"]
        for c in (ctx, twin):
            c.set_option("refit_rebuild_percent", 0)
        for k in (10, 11, 12):                                      # the sets rotate behind the rebuild
            ctx.render_enqueue(*args)
            _queued(ctx, hd, "bones", k)
            D.edit(twin, ht, "bones", k)
            twin.commit_deformed()
        _same_frame(ctx.render(*args)[0], twin.render(*args)[0], "queued calls behind a rebuild in place")
        ta, tb = ctx.mesh_trees(), twin.mesh_trees()
        assert all(ta[key].tobytes() == tb[key].tobytes() for key in ("nodes", "bsp_leaves", "tris", "tri_orig", "wide", "coarse_boxes")), "trees behind a rebuild in place"
    finally:
        twin.close()
    # commit_moved in place, and commit_lights
    _off_set_zero(ctx, hd, args, 4)
    ctx.set_option("moved_in_place", 1)
    ctx.set_transform(hd["xf"], D.slide(2))
    ctx.commit_moved()
    assert ctx.moved_commits()["full_reason"] == _capi.MOVED_NOT_FULL
    _same_frame(ctx.render(*args)[0], _fresh(fresh, builder, ("bones", 4), 4, ops=D.slide(2))[0], "commit_moved in place")
    ctx.set_positional(1, *D.point_light(3))
    ctx.commit_lights()
    _same_frame(ctx.render(*args)[0], _fresh(fresh, builder, ("bones", 4), 4, ops=D.slide(2), point=D.point_light(3))[0], "commit_lights")
    assert ctx.deform_queue()["sets"] >= 2
    # the full commit_moved, which puts the sets back to the scene's own arrays
    ctx.set_option("moved_in_place", 0)
    ctx.set_transform(hd["xf"], D.slide(3))
    ctx.commit_moved()
    assert ctx.deform_queue()["sets"] == 1
    _same_frame(ctx.render(*args)[0], _fresh(fresh, builder, ("bones", 4), 4, ops=D.slide(3), point=D.point_light(3))[0], "commit_moved, full")


@gpu
def test_deform_light_space_blocking_with_the_live_set_off_set_zero(fresh):
    """The light-space gather reads the live set's records: a blocking commit_deformed under "deform_light_space" behind queued calls
    gives the light-space bytes and the frame of a context that never queued."""
    args = D.frame_args(4)
    work, twin = ft.Context(device=0), ft.Context(device=0)
    try:
        _options((work, twin), 3)
        hw, ht = D.prepare(work, "verts"), D.prepare(twin, "verts")
        # the plane alone is edited first: the arm keeps its light-space pair
        for k in (1, 2):
            work.render_enqueue(*args)
            work.set_mesh_triangles(hw["plane"], D.plane(k))
            work.commit_deformed_enqueue()
            assert work.deform_queue()["reason"] == _capi.DEFORM_QUEUED
            twin.set_mesh_triangles(ht["plane"], D.plane(k))
            twin.commit_deformed()
        work.wait()
        assert work.deform_queue()["sets"] >= 2
        for c, h in ((work, hw), (twin, ht)):
            c.set_option("deform_light_space", 1)
            c.set_mesh_triangles(h["plane"], D.plane(3))
            c.commit_deformed()
        _same_frame(work.render(*args)[0], twin.render(*args)[0], "deform_light_space behind queued calls")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(light_space(work), light_space(twin)))
    finally:
        work.close(), twin.close()


@gpu
def test_the_hit_lists_regrow_behind_a_queued_call(fresh):
    """The scene of tests/test_pose_queue.py's regrow test with the mesh at depth 0: a non-convex mesh under CSG whose hit lists overflow
    once.  The blocking frame behind a queued deform grows them by a full commit, which goes back to the scene's own arrays; the frame
    is a fresh context's with the new vertices."""
    from .test_temporal_motion import _bunny_tris
    tris = np.asarray(_bunny_tris()).reshape(-1, 9)
    cam = ft.make_camera((0, 1, -6), (0, 0.6, 0), (0, 1, 0), H.deg(40.0))
    away = ft.make_camera((0, 1, -6), (0, 1, -12), (0, 1, 0), H.deg(40.0))      # sees nothing: its queued frame cannot overflow
    jit = ft.jitter_pattern(1)

    def bent(k):
        p = tris.reshape(-1, 3)
        q = p * np.array([1.0 + 0.04 * k, 1.0 - 0.03 * k, 1.0 + 0.02 * k]) + np.array([0.002 * k, 0.0, 0.0]) * np.sin(40.0 * p[:, 1:2])
        return np.ascontiguousarray(q.reshape(-1, 9))

    def build(b, arm_tris):
        b.clear()
        mesh = b.bsp_mesh(0, arm_tris)
        node = b.subtract(b.transform([("scale", 7.0)], mesh), b.translate((0.0, 0.9, -0.3), b.scale(0.5, b.primitive(ft.SPHERE))))
        b.set_objects(b.group([b.material(node, colour=(0.8, 0.5, 0.3), reflectance=0.2, shineyness=10)]))
        b.add_directional((-1, -1, 1), (1, 1, 1))
        b.commit()
        return mesh

    work = ft.Context(device=0)
    try:
        for c in (work, fresh):
            _options((c,), 0, csg_mesh_capacity=2)
        mesh = build(work, tris)
        work.set_mesh_triangles(mesh, bent(1))
        work.commit_deformed()                                      # the first refit since the full commit: blocking
        small = work.scene_info()["csg_capacity"]
        work.render_enqueue(away, 96, 64, 1, jit)
        work.set_mesh_triangles(mesh, bent(2))
        work.commit_deformed_enqueue()
        d = work.deform_queue()
        assert d["reason"] == _capi.DEFORM_QUEUED and d["sets"] >= 2 and d["pending"] == 1, d
        work.wait()
        got, st = work.render(cam, 96, 64, 1, jit)
        assert work.scene_info()["csg_capacity"] > small and st["csg_overflow"] == 0 and work.deform_queue()["sets"] == 1
        build(fresh, bent(2))
        want, _ = fresh.render(cam, 96, 64, 1, jit)
        _same_frame(got, want, "behind the regrown hit lists")
        assert (want != want[0, 0]).any(), "the mesh is not in the frame"
    finally:
        work.close()
        _options((fresh,), 0, csg_mesh_capacity=32)


# ---------------------------------------------------------------------------------------------------------------- 9. what may follow
@gpu
def test_what_may_follow_a_queued_call_with_a_frame_in_flight(ctx, fresh):
    _options((ctx, fresh))
    args = D.frame_args(4)
    cam, w, h, spp, jit = args
    hd = D.prepare(ctx, "bones")

    def step(k):
        ctx.render_enqueue(*args)                                   # in flight
        _queued(ctx, hd, "bones", k)
        _fresh(fresh, 0, ("bones", k), 4)
        D.build(fresh, D.expected("bones", k), D.plane())

    step(1)                                                         # the surface buffers
    ga, gb = (c.render_aov(cam, w, h, spp, jit) for c in (ctx, fresh))
    planes = [key for key in gb if isinstance(gb[key], np.ndarray)]
    assert len(planes) >= 8 and all(ga[key].tobytes() == gb[key].tobytes() for key in planes)
    step(2)                                                         # the ray queries
    o, d = H.random_rays(512, 11, origin_scale=6.0, toward=(0.2, 1.0, 0.0))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ctx.closest(o, d), fresh.closest(o, d)))
    far = np.full(len(o), 1e300)
    assert np.array_equal(ctx.blocked(o, d, far), fresh.blocked(o, d, far))
    assert np.array_equal(ctx.colour_for_ray(o, d), fresh.colour_for_ray(o, d), equal_nan=True)
    step(3)                                                         # the denoiser: its guide pass and the frame it filters
    outs = []
    for c in (ctx, fresh):
        c.render(*args, fetch=False)
        outs.append(c.denoise(cam, w, h, spp, jit)[0])
    assert outs[0].tobytes() == outs[1].tobytes()
    # a progressive accumulation is ended by the call, and a new one gives a fresh context's passes
    jit2 = ft.jitter_pattern(2)
    ctx.progressive_begin(cam, w, h)
    ctx.progressive_pass(2, jit2, seed=1, fetch=False)
    step(4)
    assert ft.hip_lib().ft_progressive_pass(ctx._ctx, 2, _capi.dptr(jit2), 2, 0, None, None) == ERR_STATE
    for c in (ctx, fresh):
        c.progressive_begin(cam, w, h)
    for seed in (1, 2):
        a, b = ctx.progressive_pass(2, jit2, seed=seed)[0], fresh.progressive_pass(2, jit2, seed=seed)[0]
        assert np.array_equal(a, b, equal_nan=True), seed
    for c in (ctx, fresh):
        c.progressive_end()


# ---------------------------------------------------------------------------------------------------------------- 10. temporal
@gpu
@pytest.mark.parametrize("form", ("accumulate", "filter"))
def test_queued_temporal_calls_with_queued_deforms_between(pinned, form):
    """Six steps of { queued deform, queued frame, queued temporal call with its own host_out } against the blocking sequence
    (commit_deformed, render, ft_temporal_accumulate [+ ft_temporal_filter]) on a second context."""
    cam, w, h, _, _ = D.frame_args(4)
    jit = np.zeros((1, 2))
    calls = 6
    filt = dict(demodulate=1) if form == "filter" else None
    ring = pinned((h, w, 3), calls)
    blocking, queued = ft.Context(device=0), ft.Context(device=0)
    try:
        _options((blocking, queued))
        hb, hq = D.prepare(blocking, "bones"), D.prepare(queued, "bones")

        def deform_blocking(k):
            if k:
                D.edit(blocking, hb, "bones", k)
                blocking.commit_deformed()

        def deform_queued(k):
            if k:
                _queued(queued, hq, "bones", k, what=form)
            return False                                            # (nothing was retired)

        outs, final, _ = TQ._blocking(blocking, [cam] * calls, 1, jit, None, filt, False, w=w, h=h, seed0=900, between=deform_blocking)
        got, _ = TQ._queued(queued, [cam] * calls, 1, jit, None, filt, False, ring, w=w, h=h, seed0=900, between=deform_queued, want=outs, what=form)
        TQ._same_final(got, final, form)
        assert final["status"]["calls"] == calls and final["status"]["with_history"] > 0
        counted = queued.deform_queue()
        assert counted["queued"] == calls - 1 and counted["blocking"] == 0, counted
        assert counted["pending"] >= 2 and counted["sets"] <= _capi.GEO_SETS_MAX, counted   # frames and temporal calls in flight at the last call
        assert any(D.changed(a, b) >= D.MIN_CHANGED_FRACTION * w * h for a, b in zip(outs, outs[1:]))
        queued.temporal_end(), blocking.temporal_end()
    finally:
        blocking.close(), queued.close()


# ---------------------------------------------------------------------------------------------------------------- 11. unused
@gpu
def test_a_context_that_never_queues_a_deform_is_unchanged():
    """Two runs of blocking commit_deformed poses: frames, light-space arrays and mesh trees as they lie in device memory are the same
    bytes, and the context holds the scene's own arrays alone."""
    args = D.frame_args(4)
    runs = []
    for _ in range(2):
        c = ft.Context(device=0)
        try:
            _options((c,), 3)
            hd = D.prepare(c, "bones")
            seen = []
            for k in range(1, 5):
                D.edit(c, hd, "bones", k)
                c.commit_deformed()
                seen.append(c.render(*args)[0].tobytes())
                seen += [a.tobytes() for a in light_space(c)]
                trees = c.mesh_trees()
                seen += [trees[key].tobytes() for key in ("nodes", "bsp_leaves", "tris", "wide", "coarse_boxes")]
            assert c.deform_queue() == dict(ZEROS, sets=1)
            runs.append(seen)
        finally:
            c.close()
    assert runs[0] == runs[1]

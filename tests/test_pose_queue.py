"""Queued pose and light commits (include/functracer_hip.h "queued pose and light commits"):
ft_scene_commit_moved_enqueue and ft_scene_commit_lights_enqueue commit new poses or light values without retiring a queued frame or
draining a stream, through the sequences of tests/pose_queue_tools.py and tests/move_tools.py.

The CPU half checks the entry points, that a host-only context takes the full host commit with reason 1 and the twins' FT_ERR_STATE
rules, and on the oracle alone that every step of every new sequence changes at least 20 pixels.

The GPU half: a step is { setters, queued commit, queued frame into its own page-locked buffer }, twelve of them before one wait, and
frame k must be bitwise what a context built from scratch at step k renders - so a commit that reached the device too early or too late,
or a pose set handed out while a frame still read it, shows as a wrong frame.  Then everything that may follow a queued commit, every
fallback with its reason code, every other commit after a queued one has moved the live pose set, lights, the queued temporal calls, a
two-device context, and a context that never uses the feature."""
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
from . import pose_queue_tools as Q
from . import shadow_tools as S
from . import walk_tools as W
from . import test_temporal_motion as M
from . import test_temporal_queue as TQ
from .test_light_space_shadows import light_space
from .test_moved_in_place import _state

gpu = pytest.mark.gpu
ERR_INVALID, ERR_STATE = -1, -5
ZEROS = dict(zip(_capi.POSE_QUEUE_FIELDS, [0] * 8))


# =============================================================================================================================
# CPU half

def test_header_declares_and_library_exports_the_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    lib = ft.hip_lib()
    for decl, name in (("int32_t ft_scene_commit_moved_enqueue(ft_context* ctx);", "ft_scene_commit_moved_enqueue"),
                       ("int32_t ft_scene_commit_lights_enqueue(ft_context* ctx);", "ft_scene_commit_lights_enqueue"),
                       ("int32_t ft_debug_pose_queue(ft_context* ctx, int64_t out[8]);", "ft_debug_pose_queue")):
        assert decl in hdr and hasattr(lib, name), name
    assert lib.ft_abi_version() == 2 and "#define FT_ABI_VERSION 2" in hdr      # additions only
    assert all(callable(getattr(ft.Context, k)) for k in ("commit_moved_enqueue", "commit_lights_enqueue", "pose_queue"))
    assert _capi.POSE_SETS_MAX == Q.FRAME_SLOTS + _capi.TEMPORAL_QUEUE_DEPTH + 1 == 9 and "up to 9 copies" in hdr


def test_null_arguments():
    lib = ft.hip_lib()
    out = (C.c_int64 * 8)()
    assert lib.ft_scene_commit_moved_enqueue(None) == ERR_INVALID and lib.ft_scene_commit_lights_enqueue(None) == ERR_INVALID
    ctx = ft.Context(host_only=True)
    assert lib.ft_debug_pose_queue(None, out) == ERR_INVALID and lib.ft_debug_pose_queue(ctx._ctx, None) == ERR_INVALID
    assert ctx.pose_queue() == ZEROS
    ctx.close()


@pytest.mark.parametrize("seq", (Q.SLIDES, Q.HAND))
def test_host_only_moved_call_takes_the_full_commit(seq):
    """Byte for byte the blocking twin's scene, counted as a call that took the blocking path with reason 1; no pose set exists."""
    ctx, twin = ft.Context(host_only=True), ft.Context(host_only=True)
    steps = Q.sequence(seq)
    hd, ht = Q.build(ctx, seq, steps[0]), Q.build(twin, seq, steps[0])
    for k, step in enumerate(steps[1:4], 1):
        MV.move(ctx, hd, step["pose"], commit=False)
        ctx.commit_moved_enqueue()
        MV.move(twin, ht, step["pose"])
        assert _state(ctx) == _state(twin), (seq, k)
        assert ctx.pose_queue() == dict(ZEROS, moved_blocking=k, moved_reason=_capi.POSE_HOST_ONLY), (seq, k)
    assert ctx.moved_commits() == twin.moved_commits()
    ctx.close(), twin.close()


def test_host_only_lights_call_takes_the_full_commit():
    ctx, twin = ft.Context(host_only=True), ft.Context(host_only=True)
    steps = Q.sequence(Q.LIGHTS)
    Q.build(ctx, Q.LIGHTS, steps[0]), Q.build(twin, Q.LIGHTS, steps[0])
    for k, step in enumerate(steps[1:4], 1):
        L.set_lights(ctx, step["lights"])
        ctx.commit_lights_enqueue()
        L.set_lights(twin, step["lights"])
        twin.commit_lights()
        assert _state(ctx) == _state(twin), k
        assert ctx.pose_queue() == dict(ZEROS, lights_blocking=k, lights_reason=_capi.POSE_HOST_ONLY), k
    ctx.close(), twin.close()


def test_state_rules_are_the_twins():
    """Each refusal of a twin, in the twin's order, is the queued call's: the same code from the same state, nothing counted."""
    lib = ft.hip_lib()
    moved = (lib.ft_scene_commit_moved, lib.ft_scene_commit_moved_enqueue)
    lights = (lib.ft_scene_commit_lights, lib.ft_scene_commit_lights_enqueue)
    steps = Q.sequence(Q.SLIDES)

    def both(calls, prepare):
        codes = []
        for call in calls:
            c = ft.Context(host_only=True)
            prepare(c)
            codes.append(call(c._ctx))
            assert c.pose_queue() == ZEROS
            c.close()
        assert codes[0] == codes[1] == ERR_STATE, codes

    def held(c):
        return Q.build(c, Q.SLIDES, steps[0])

    for calls in (moved, lights):
        both(calls, lambda c: None)                                 # no held commit
        both(calls, lambda c: (held(c), c.primitive(ft.SPHERE)))    # a structural change
        both(calls, lambda c: (held(c), c.add_directional((0, -1, 0), (1, 1, 1))))
    both(lights, lambda c: c.set_transform(held(c)[0], [("translate", (0.1, 0.0, 0.0))]))       # a pending transform
    tris = S.mesh_tris(S.CASES["multi-leaf"].parts[0][0]).reshape(-1, 9)
    both(lights, lambda c: c.set_mesh_triangles(held(c)["meshes"][0], tris * 1.01))             # pending vertices
    both(lights, lambda c: (held(c), c.set_option("light_space_shadows", 1)))                   # a commit-time option


@pytest.mark.parametrize("seq", Q.SEQUENCES)
def test_every_step_changes_the_frame_on_the_oracle(seq):
    """A condition on the reference alone, so that the ordering tests are not vacuous: consecutive steps differ in at least 20 pixels
    (move_tools.oracle_steps proves the same for the sequences of tests/move_tools.py), and the lights sequence does so by its lights
    alone, with the objects left where they were."""
    frames = Q.oracle_frames(seq)
    counts = [Q.changed(a, b) for a, b in zip(frames, frames[1:])]
    print(f"{seq}: pixels changed per step {counts}")
    assert len(counts) == Q.STEPS and min(counts) >= Q.MIN_CHANGED, (seq, counts)
    if seq == Q.LIGHTS:
        frames = Q.oracle_frames(seq, True)
        counts = [Q.changed(a, b) for a, b in zip(frames, frames[1:])]
        print(f"{seq}, the lights alone: pixels changed per step {counts}")
        assert min(counts) >= Q.MIN_CHANGED, counts


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

    def get(shape, n=Q.STEPS):
        have = made.setdefault(tuple(shape), [])
        while len(have) < n:
            have.append(ft.PinnedArray(shape, np.float64))
        return [p.array for p in have[:n]]

    yield get
    for ps in made.values():
        for p in ps:
            p.close()


def _options(contexts, shadows=2, **more):
    for c in contexts:
        c.set_option("light_space_shadows", shadows)
        for k, v in more.items():
            c.set_option(k, v)


def _counters(st):
    return {k: v for k, v in L.counters(st).items() if k != "n_launches"}     # (the level hint restarts: n_launches depends on it)


_FRESH = {}


def _fresh_frames(fresh, seq, spp, shadows=2):
    """[(frame, counters)] of steps 1 .. STEPS on a context built from scratch at each: computed once, shared, never changed."""
    key = (seq, spp, shadows)
    if key not in _FRESH:
        _options((fresh,), shadows)
        args, tiles = Q.frame_args(seq, spp)
        out = []
        for step in Q.sequence(seq)[1:]:
            Q.build(fresh, seq, step)
            frame, st = fresh.render(*args, tiles=tiles)
            frame.setflags(write=False)
            out.append((frame, _counters(st)))
        _options((fresh,))
        _FRESH[key] = out
    return _FRESH[key]


def _delta(ctx, before):
    now = ctx.pose_queue()
    return {k: now[k] - before[k] if k.endswith(("queued", "blocking")) else now[k] for k in now}


def _run_queued(c, seq, spp, bufs):
    """STEPS steps of { setters, queued commits, queued frame into its own buffer }, then one wait.  Returns the last frame's statistics
    and what ft_debug_pose_queue counted."""
    steps = Q.sequence(seq)
    hd = Q.build(c, seq, steps[0])
    args, tiles = Q.frame_args(seq, spp)
    before = c.pose_queue()
    for k, step in enumerate(steps[1:]):
        Q.set_step(c, hd, step)
        bufs[k][...] = 0.0
        c.render_enqueue(*args, tiles=tiles, out=bufs[k])
    st = c.wait()
    return st, _delta(c, before)


def _check_run(seq, spp, bufs, st, counted, want, what):
    for k, (frame, _) in enumerate(want):
        assert np.array_equal(bufs[k], frame, equal_nan=True), f"{what}: frame {k + 1} is not the fresh context's ({Q.changed(bufs[k], frame)} pixels differ)"
    assert _counters(st) == want[-1][1], what
    lights = Q.sequence(seq)[1]["lights"] is not None
    assert counted["moved_queued"] == Q.STEPS and counted["moved_blocking"] == 0 and counted["moved_reason"] == _capi.POSE_QUEUED, (what, counted)
    assert counted["lights_queued"] == (Q.STEPS if lights else 0) and counted["lights_blocking"] == 0, (what, counted)
    # the host retired nothing for the commits: when the last one returned, the frames of the steps before it were still pending
    assert counted["pending"] == Q.pending_at_last_call(Q.STEPS - 1) == Q.FRAME_SLOTS, (what, counted)
    assert 2 <= counted["sets"] <= _capi.POSE_SETS_MAX, (what, counted)


# ---------------------------------------------------------------------------------------------------------------- 1. ordering
@gpu
@pytest.mark.parametrize("seq,spp", ((Q.SLIDES, MV.SPP), (Q.HAND, MV.SPP), (Q.HAND, 16)))
def test_twelve_queued_steps_each_frame_a_fresh_contexts(ctx, fresh, pinned, seq, spp):
    """More steps than pose sets, so sets are reused while frames are in flight; at 160 x 90 x 16 the frames really overlap the uploads."""
    _options((ctx,))
    args, _ = Q.frame_args(seq, spp)
    bufs = pinned((args[2], args[1], 3))
    want = _fresh_frames(fresh, seq, spp)
    st, counted = _run_queued(ctx, seq, spp, bufs)
    print(f"{seq} x{spp}: {counted}")
    _check_run(seq, spp, bufs, st, counted, want, f"{seq} x{spp}")
    times = ctx.commit_times()
    assert times["device_bvh_ms"] == 0.0 and times["flatten_ms"] > 0.0 and times["upload_ms"] > 0.0, times


# ---------------------------------------------------------------------------------------------------------------- 2. what may follow
def _same(c, fresh, name, what, spp=MV.SPP):
    a, sa = MV.render(c, name, spp)
    b, sb = MV.render(fresh, name, spp)
    assert np.array_equal(a, b, equal_nan=True), f"{what} x{spp}: {Q.changed(a, b)} pixels differ from the fresh context"
    assert _counters(sa) == _counters(sb), f"{what} x{spp}"
    return a


def _same_surfaces(c, fresh, name, what):
    ga, gb = MV.render_aov(c, name), MV.render_aov(fresh, name)
    planes = [key for key in gb if isinstance(gb[key], np.ndarray)]
    assert len(planes) >= 8 and all(ga[key].tobytes() == gb[key].tobytes() for key in planes), what
    assert all(x.tobytes() == y.tobytes() for x, y in zip(c.leaf_matrices(), fresh.leaf_matrices())), what


def _queued_move(c, hd, pose, reason=_capi.POSE_QUEUED, what=""):
    before = c.pose_queue()
    MV.move(c, hd, pose, commit=False)
    c.commit_moved_enqueue()
    d = _delta(c, before)
    assert d["moved_reason"] == reason and (d["moved_queued"], d["moved_blocking"]) == ((1, 0) if reason == _capi.POSE_QUEUED else (0, 1)), (what, d)
    return d


@gpu
@pytest.mark.parametrize("seq", (Q.SLIDES, Q.HAND))
def test_blocking_calls_after_queued_moves(ctx, fresh, seq):
    """Several moves with no frame between them, then a frame; then every kind of blocking call behind a queued move."""
    _options((ctx, fresh))
    name = Q.scene_of(seq)
    steps = Q.sequence(seq)
    args, tiles = Q.frame_args(seq, 1)
    hd = Q.build(ctx, seq, steps[0])
    ctx.render_enqueue(*args, tiles=tiles)                          # in flight under the first of them
    for step in steps[1:6]:
        _queued_move(ctx, hd, step["pose"], what=seq)
    Q.build(fresh, seq, steps[5])
    _same(ctx, fresh, name, f"{seq}: five moves, then a frame")
    _same_surfaces(ctx, fresh, name, f"{seq}: five moves, then a frame")
    # the surface buffers first, with a frame still in flight
    ctx.render_enqueue(*args, tiles=tiles)
    _queued_move(ctx, hd, steps[6]["pose"], what=seq)
    Q.build(fresh, seq, steps[6])
    _same_surfaces(ctx, fresh, name, f"{seq}: surfaces behind a queued move")
    # the ray queries
    ctx.render_enqueue(*args, tiles=tiles)
    _queued_move(ctx, hd, steps[7]["pose"], what=seq)
    Q.build(fresh, seq, steps[7])
    if name == Q.HAND:
        o, d = H.random_rays(512, 11, origin_scale=6.0, toward=(-2.0, 1.5, 0.0))
    else:
        o, d, _, _ = W.pixel_rays(S.view_of(S.CASES[name]))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ctx.closest(o, d), fresh.closest(o, d))), seq
    far = np.full(len(o), 1e300)
    assert np.array_equal(ctx.blocked(o, d, far), fresh.blocked(o, d, far)), seq
    assert np.array_equal(ctx.colour_for_ray(o, d), fresh.colour_for_ray(o, d), equal_nan=True), seq
    # a progressive accumulation is ended by the call, and a new one gives a fresh context's passes
    cam, w, h = args[0], args[1], args[2]
    jit2 = ft.jitter_pattern(2)
    ctx.progressive_begin(cam, w, h, tiles=tiles)
    ctx.progressive_pass(2, jit2, seed=1, fetch=False)
    _queued_move(ctx, hd, steps[8]["pose"], what=seq)
    assert ft.hip_lib().ft_progressive_pass(ctx._ctx, 2, _capi.dptr(jit2), 2, 0, None, None) == ERR_STATE
    Q.build(fresh, seq, steps[8])
    for c in (ctx, fresh):
        c.progressive_begin(cam, w, h, tiles=tiles)
    for seed in (1, 2):
        a, b = ctx.progressive_pass(2, jit2, seed=seed)[0], fresh.progressive_pass(2, jit2, seed=seed)[0]
        assert np.array_equal(a, b, equal_nan=True), (seq, seed)
    for c in (ctx, fresh):
        c.progressive_end()
    # the denoiser: its guide pass and the frame it filters
    ctx.render_enqueue(*args, tiles=tiles)
    _queued_move(ctx, hd, steps[9]["pose"], what=seq)
    Q.build(fresh, seq, steps[9])
    outs = []
    for c in (ctx, fresh):
        MV.render(c, name, MV.SPP, fetch=False)
        outs.append(c.denoise(cam, w, h, MV.SPP, S.jitter(MV.SPP), tiles=tiles)[0])
    assert np.array_equal(outs[0], outs[1], equal_nan=True), seq


# ---------------------------------------------------------------------------------------------------------------- 3. fallbacks
@gpu
@pytest.mark.parametrize("shadows", (0, 1, 2))
def test_turning_mesh_leaves_fall_back_unless_no_pair_exists(ctx, fresh, pinned, shadows):
    """move_tools' multi-leaf sequence: slides are queued whatever the option says; with light-space structures a turn changes a pair's
    frame and the call takes the blocking path (reason 4), without them everything is queued.  Either way the bits are a fresh context's,
    and the frame queued in front of each call shows the pose before it."""
    _options((ctx, fresh), shadows)
    name = "multi-leaf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps = MV.sequence(name)
    hd = MV.build(ctx, case, steps[0][2])
    buf = pinned((view.h, view.w, 3), 1)[0]
    MV.build(fresh, case, steps[0][2])
    previous = _same(ctx, fresh, name, "the committed pose")
    for k, (kind, what, pose) in enumerate(steps[1:], 1):
        label = f"multi-leaf shadows {shadows} step {k} ({what})"
        buf[...] = 0.0
        ctx.render_enqueue(W.camera(view), view.w, view.h, MV.SPP, S.jitter(MV.SPP), tiles=view.tiles, out=buf)
        before = ctx.pose_queue()
        MV.move(ctx, hd, pose, commit=False)
        ctx.commit_moved_enqueue()
        d = _delta(ctx, before)
        assert d["moved_queued"] + d["moved_blocking"] == 1 and d["moved_reason"] in (_capi.POSE_QUEUED, _capi.POSE_PAIR_CHANGED), (label, d)
        if shadows == 0 or k == 1:                                  # (step 1 slides from the committed pose; the later slides also undo a turn or a scale)
            assert d["moved_reason"] == _capi.POSE_QUEUED and d["pending"] == 1, (label, d)
        elif kind == MV.TURN:
            assert d["moved_reason"] == _capi.POSE_PAIR_CHANGED and d["pending"] == 0, (label, d)
        MV.build(fresh, case, pose)
        frame = _same(ctx, fresh, name, label)                      # (retires the queued frame)
        assert np.array_equal(buf, previous, equal_nan=True), f"{label}: the frame queued before the call does not show the old pose"
        _same_surfaces(ctx, fresh, name, label)
        if d["moved_reason"] == _capi.POSE_PAIR_CHANGED and kind != MV.SINGULAR:
            L.check_structures(ctx, case, L.initial(case), grids=shadows == 2)
        previous = frame
    _options((ctx, fresh))


@gpu
def test_pending_edits_take_the_full_commit_with_reason_2(ctx, fresh):
    _options((ctx, fresh))
    name = "two_clusters"
    case = S.CASES[name]
    steps, lights = MV.sequence(name), L.sequence(name)
    args = (W.camera(S.view_of(case)), S.view_of(case).w, S.view_of(case).h, 1, S.jitter(1))
    hd = MV.build(ctx, case, steps[0][2])
    tris = S.mesh_tris(case.parts[0][0]).reshape(-1, 9)
    bent = tris * np.array([1.0, 1.04, 1.0] * 3)
    ctx.render_enqueue(*args, tiles=S.view_of(case).tiles)
    L.set_lights(ctx, lights[3][1])                                 # a light setter
    d = _queued_move(ctx, hd, steps[1][2], _capi.POSE_PENDING, "a pending light setter")
    assert d["pending"] == 0 and d["sets"] == 1
    MV.build(fresh, case, steps[1][2], lights=lights[3][1])
    _same(ctx, fresh, name, "a pending light setter")
    ctx.set_mesh_triangles(hd["meshes"][0], bent)                   # new vertices
    _queued_move(ctx, hd, steps[8][2], _capi.POSE_PENDING, "pending vertices")
    MV.build(fresh, case, steps[8][2], lights=lights[3][1], tris={0: bent})
    _same(ctx, fresh, name, "pending vertices")
    _options((ctx, fresh), 1)                                       # a commit-time option
    _queued_move(ctx, hd, steps[1][2], _capi.POSE_PENDING, "a pending commit-time option")
    MV.build(fresh, case, steps[1][2], lights=lights[3][1], tris={0: bent})
    _same(ctx, fresh, name, "a pending commit-time option")
    _queued_move(ctx, hd, steps[8][2], what="nothing pending any more")   # a slide: queued again
    MV.build(fresh, case, steps[8][2], lights=lights[3][1], tris={0: bent})
    _same(ctx, fresh, name, "nothing pending any more")
    _options((ctx, fresh))


@gpu
def test_an_item_past_six_face_directions_takes_the_full_commit_with_reason_3(ctx, fresh):
    _options((ctx, fresh))
    hd = MV.build_union(ctx, MV.union_pose())
    cam, w, h = MV.union_camera(), MV.UNION_CAM["w"], MV.UNION_CAM["h"]
    for what, pose, reason in (("slid", MV.union_pose(whole=(0.5, 1.0, 0.0)), _capi.POSE_QUEUED),
                               ("the union turned", MV.union_pose(b_deg=50.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), _capi.POSE_QUEUED),
                               ("C turned: past six", MV.union_pose(b_deg=50.0, c_deg=20.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), _capi.POSE_DIFFERS),
                               ("C turned further", MV.union_pose(b_deg=50.0, c_deg=35.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), _capi.POSE_QUEUED),
                               ("C back: five again", MV.union_pose(b_deg=50.0, whole=(0.5, 1.0, 0.0), whole_deg=40.0), _capi.POSE_DIFFERS)):
        ctx.render_enqueue(cam, w, h, 1, S.jitter(1))
        d = _queued_move(ctx, hd, pose, reason, what)
        assert d["pending"] == (1 if reason == _capi.POSE_QUEUED else 0), (what, d)
        MV.build_union(fresh, pose)
        for spp in (1, MV.SPP):
            a, sa = ctx.render(cam, w, h, spp, S.jitter(spp))
            b, sb = fresh.render(cam, w, h, spp, S.jitter(spp))
            assert np.array_equal(a, b, equal_nan=True) and _counters(sa) == _counters(sb), f"{what} x{spp}"
        assert sorted(ctx.scene_info().items()) == sorted(fresh.scene_info().items()), what


# ---------------------------------------------------------------------------------------------------------------- 4. mixing
def _translated(pose, keys, by):
    out = {k: list(v) for k, v in pose.items()}
    for k in keys:
        out[k] = out[k] + [("translate", by)]
    return out


@gpu
def test_every_other_commit_after_the_live_set_has_moved(ctx, fresh):
    """A frame in flight holds the live pose set when a queued move arrives, so the move goes to another set, which becomes the live one.
    From that state: the blocking commit_moved (in place and full), commit_lights, commit_deformed (with and without
    "deform_light_space") and a full commit.  The blocking partial commits must write the LIVE set, the full ones go back to the first."""
    _options((ctx, fresh), moved_in_place=1, deform_light_space=0)
    name = "multi-leaf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps, lights = MV.sequence(name), L.sequence(name)
    movers = MV.MOVERS[name]
    state = dict(pose=steps[0][2], lights=None, tris=None)
    hd = MV.build(ctx, case, state["pose"])

    def elsewhere(k):
        ctx.render_enqueue(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
        state["pose"] = _translated(state["pose"], movers, (0.01 * k, 0.0, -0.02))
        d = _queued_move(ctx, hd, state["pose"], what=f"leaving the live set, {k}")
        assert d["sets"] >= 2 and d["pending"] == 1, d              # the frame held the live set: the move took another

    def same(what):
        MV.build(fresh, case, state["pose"], lights=state["lights"], tris=state["tris"])
        _same(ctx, fresh, name, what)
        _same_surfaces(ctx, fresh, name, what)

    try:
        elsewhere(1)
        same("a queued move alone")
        elsewhere(2)
        state["pose"] = steps[3][2]                                 # turned 30 degrees
        MV.move(ctx, hd, state["pose"])
        assert ctx.moved_commits()["full_reason"] == _capi.MOVED_NOT_FULL and ctx.pose_queue()["sets"] >= 2
        same("commit_moved in place after a queued move")
        L.check_structures(ctx, case, L.initial(case))
        elsewhere(3)
        ctx.set_option("moved_in_place", 0)
        state["pose"] = steps[4][2]
        MV.move(ctx, hd, state["pose"])
        assert ctx.moved_commits()["full_reason"] == _capi.MOVED_OPTION_OFF and ctx.pose_queue()["sets"] == 1
        same("the full commit_moved after a queued move")
        elsewhere(4)
        state["lights"] = lights[3][1]                              # both directional lights tilted
        L.set_lights(ctx, state["lights"])
        ctx.commit_lights()
        assert ctx.pose_queue()["sets"] >= 2
        same("commit_lights after a queued move")
        L.check_structures(ctx, case, state["lights"])
        tris = S.mesh_tris(case.parts[0][0]).reshape(-1, 9)
        for k, (option, bent) in enumerate(((0, tris * np.array([1.0, 1.05, 0.97] * 3)), (1, tris * np.array([1.1, 0.9, 1.0] * 3)))):
            elsewhere(5 + k)
            for c in (ctx, fresh):
                c.set_option("deform_light_space", option)          # (not a commit-time option)
            state["tris"] = {0: bent}
            ctx.set_mesh_triangles(hd["meshes"][0], bent)
            ctx.commit_deformed()
            assert ctx.pose_queue()["sets"] >= 2
            same(f"commit_deformed after a queued move, deform_light_space {option}")
        elsewhere(7)
        ctx.commit()                                                # nothing pending: the full commit of the graph as it stands
        assert ctx.pose_queue()["sets"] == 1
        same("a full commit after a queued move")
        elsewhere(8)                                                # and the feature works again from there
        same("a queued move after the full commit")
    finally:
        _options((ctx, fresh), moved_in_place=0, deform_light_space=0)


@gpu
def test_the_hit_lists_regrow_after_a_queued_move(ctx, fresh):
    """A mesh under CSG with hit lists that overflow once: the blocking frame behind a queued move grows them by a full commit, which goes
    back to the first pose set; the frame is a fresh context's at the new pose."""
    tris = np.asarray(M._bunny_tris()).reshape(-1, 9)
    cam = ft.make_camera((0, 1, -6), (0, 0.6, 0), (0, 1, 0), H.deg(40.0))
    away = ft.make_camera((0, 1, -6), (0, 1, -12), (0, 1, 0), H.deg(40.0))      # sees nothing: its queued frame cannot overflow
    jit = ft.jitter_pattern(1)

    def build(b, at):
        b.clear()
        hd = b.transform([("scale", 7.0), ("translate", at)], b.bsp_mesh(3, tris))
        node = b.subtract(hd, b.translate((0.0, 0.9, -0.3), b.scale(0.5, b.primitive(ft.SPHERE))))
        b.set_objects(b.group([b.material(node, colour=(0.8, 0.5, 0.3), reflectance=0.2, shineyness=10)]))
        b.add_directional((-1, -1, 1), (1, 1, 1))
        b.commit()
        return hd

    try:
        _options((ctx, fresh), csg_mesh_capacity=2)
        hd = build(ctx, (0.0, 0.0, 0.0))
        small = ctx.scene_info()["csg_capacity"]
        ctx.render_enqueue(away, 96, 64, 1, jit)
        before = ctx.pose_queue()
        ctx.set_transform(hd, [("scale", 7.0), ("translate", (0.15, 0.0, 0.1))])
        ctx.commit_moved_enqueue()
        d = _delta(ctx, before)
        assert d["moved_reason"] == _capi.POSE_QUEUED and d["sets"] >= 2 and d["pending"] == 1, d
        ctx.wait()
        got, st = ctx.render(cam, 96, 64, 1, jit)
        assert ctx.scene_info()["csg_capacity"] > small and st["csg_overflow"] == 0 and ctx.pose_queue()["sets"] == 1
        build(fresh, (0.15, 0.0, 0.1))
        want, _ = fresh.render(cam, 96, 64, 1, jit)
        assert np.array_equal(got, want, equal_nan=True)
    finally:
        _options((ctx, fresh), csg_mesh_capacity=32)


# ---------------------------------------------------------------------------------------------------------------- 5. lights
@gpu
def test_twelve_queued_light_and_pose_steps(ctx, fresh, pinned):
    """The point light, a directional light's colour and the soft light's scatter change every frame, beside casters that slide every
    frame: both commits are queued at every step."""
    _options((ctx,))
    args, _ = Q.frame_args(Q.LIGHTS, MV.SPP)
    bufs = pinned((args[2], args[1], 3))
    want = _fresh_frames(fresh, Q.LIGHTS, MV.SPP)
    st, counted = _run_queued(ctx, Q.LIGHTS, MV.SPP, bufs)
    print(f"{Q.LIGHTS}: {counted}")
    _check_run(Q.LIGHTS, MV.SPP, bufs, st, counted, want, Q.LIGHTS)


@gpu
@pytest.mark.parametrize("shadows", (1, 2))
def test_a_directional_light_that_turns_over_a_mesh_with_pairs_falls_back(ctx, fresh, shadows):
    _options((ctx, fresh), shadows)
    name = "blob(65)-mirror"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    twin = ft.Context(device=0)
    try:
        _options((twin,), shadows)
        lights = L.sequence(name)
        L.build(ctx, case, lights[0][1]), L.build(twin, case, lights[0][1])
        for what, ls in lights[1:5]:
            ctx.render_enqueue(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
            before = ctx.pose_queue()
            L.set_lights(ctx, ls)
            ctx.commit_lights_enqueue()
            d = _delta(ctx, before)
            assert (d["lights_queued"], d["lights_blocking"], d["lights_reason"], d["pending"]) == (0, 1, _capi.POSE_PAIR_CHANGED, 0), (what, d)
            L.set_lights(twin, ls)
            twin.commit_lights()
            L.build(fresh, case, ls)
            a = _same(ctx, fresh, name, f"shadows {shadows}: {what}")
            assert np.array_equal(a, MV.render(twin, name, MV.SPP)[0], equal_nan=True), what
            assert all(x.tobytes() == y.tobytes() for x, y in zip(light_space(ctx), light_space(twin))), what
            L.check_structures(ctx, case, ls, grids=shadows == 2)
    finally:
        twin.close()
        _options((ctx, fresh))


@gpu
def test_a_directional_light_turns_queued_over_primitives(ctx, fresh):
    _options((ctx, fresh))
    hd = MV.build_union(ctx, MV.union_pose())
    MV.build_union(fresh, MV.union_pose())
    cam, w, h = MV.union_camera(), MV.UNION_CAM["w"], MV.UNION_CAM["h"]
    previous = None
    for k, v in enumerate(((0.5, -1.0, 0.1), (-0.4, -1.0, 0.3), (0.1, -1.0, -0.6)), 1):
        ctx.render_enqueue(cam, w, h, 1, S.jitter(1))
        before = ctx.pose_queue()
        ctx.set_directional(0, v, (1.0, 1.0 - 0.1 * k, 1.0))
        ctx.commit_lights_enqueue()
        d = _delta(ctx, before)
        assert (d["lights_queued"], d["lights_blocking"], d["lights_reason"], d["pending"]) == (1, 0, _capi.POSE_QUEUED, 1), d
        fresh.set_directional(0, v, (1.0, 1.0 - 0.1 * k, 1.0))
        fresh.commit()
        a, sa = ctx.render(cam, w, h, MV.SPP, S.jitter(MV.SPP))
        b, sb = fresh.render(cam, w, h, MV.SPP, S.jitter(MV.SPP))
        assert np.array_equal(a, b, equal_nan=True) and _counters(sa) == _counters(sb), k
        assert previous is None or Q.changed(a, previous) >= Q.MIN_CHANGED
        previous = a
    assert hd


# ---------------------------------------------------------------------------------------------------------------- 6. temporal
@gpu
@pytest.mark.parametrize("form", ("accumulate", "filter", "clamp"))
@pytest.mark.parametrize("which", ("sliding sphere", "mixed"))
def test_queued_temporal_calls_with_queued_moves_between(pinned, which, form):
    """The six-call sequences of tests/test_temporal_motion.py: per call a queued move, a queued frame and a queued temporal call with
    its own host_out, against the blocking sequence (commit_moved in place, render, ft_temporal_accumulate [+ ft_temporal_filter]) on a
    second context.  "mixed" turns the mesh, so it runs under "light_space_shadows" 0, where nothing has a pair."""
    cam, jit = M._camera(), np.zeros((1, 2))
    pose = (lambda k: M._pose(float(k), sphere_only=True, sphere_step=0.4)) if which == "sliding sphere" else (lambda k: M._pose(float(k)))
    filt = dict(demodulate=1) if form == "filter" else None
    clamp = 1 if form == "clamp" else None
    shadows = 2 if which == "sliding sphere" else 0
    ring = pinned((M.Hh, M.W, 3), M.CALLS)
    blocking, queued = ft.Context(device=0), ft.Context(device=0)
    try:
        _options((blocking, queued), shadows, moved_in_place=1)
        hb, hq = M._build(blocking, pose(0)), M._build(queued, pose(0))

        def move_blocking(k):
            if k:
                MV.move(blocking, hb, pose(k))

        def move_queued(k):
            if k:
                MV.move(queued, hq, pose(k), commit=False)
                queued.commit_moved_enqueue()
            return False                                            # (nothing was retired)

        outs, final, _ = TQ._blocking(blocking, [cam] * M.CALLS, 1, jit, None, filt, False, clamp=clamp, w=M.W, h=M.Hh, seed0=700, between=move_blocking)
        got, _ = TQ._queued(queued, [cam] * M.CALLS, 1, jit, None, filt, False, ring, clamp=clamp, w=M.W, h=M.Hh, seed0=700, between=move_queued, want=outs,
                            what=f"{which}, {form}")
        TQ._same_final(got, final, f"{which}, {form}")
        assert final["status"]["calls"] == M.CALLS and final["status"]["with_history"] > 0
        counted = queued.pose_queue()
        assert counted["moved_queued"] == M.CALLS - 1 and counted["moved_blocking"] == 0, counted
        assert counted["pending"] >= 2 and counted["sets"] <= _capi.POSE_SETS_MAX, counted   # frames and temporal calls in flight at the last move
        assert any(Q.changed(a, b) >= Q.MIN_CHANGED for a, b in zip(outs, outs[1:]))
        queued.temporal_end(), blocking.temporal_end()
    finally:
        blocking.close(), queued.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the rest
@gpu
def test_two_device_context_on_one_gpu(fresh, pinned):
    two = ft.Context(device=[0, 0])
    try:
        _options((two,))
        args, _ = Q.frame_args(Q.SLIDES, MV.SPP)
        bufs = pinned((args[2], args[1], 3))
        want = _fresh_frames(fresh, Q.SLIDES, MV.SPP)
        _, counted = _run_queued(two, Q.SLIDES, MV.SPP, bufs)
        for k, (frame, _) in enumerate(want):
            assert np.array_equal(bufs[k], frame, equal_nan=True), f"[0, 0]: frame {k + 1} ({Q.changed(bufs[k], frame)} pixels differ)"
        assert counted["moved_queued"] == Q.STEPS and counted["moved_blocking"] == 0 and counted["pending"] == Q.FRAME_SLOTS, counted
    finally:
        two.close()


@gpu
def test_a_kept_classification_is_not_reused_across_a_queued_call(ctx, fresh):
    _options((ctx, fresh))
    name = "blob(65)-mirror"
    case = S.CASES[name]
    steps = MV.sequence(name)
    hd = MV.build(ctx, case, steps[0][2])
    for _ in range(2 * Q.FRAME_SLOTS):                              # every slot keeps the view's classification
        MV.render(ctx, name, 1)
    reuse = ctx.classify_reuse()
    for _ in range(Q.FRAME_SLOTS):
        MV.render(ctx, name, 1)
    after = ctx.classify_reuse()
    assert after["reused"] == reuse["reused"] + Q.FRAME_SLOTS and after["classified"] == reuse["classified"], (reuse, after)
    _queued_move(ctx, hd, steps[1][2])                              # a slide: queued, and still another scene
    for _ in range(Q.FRAME_SLOTS):
        MV.render(ctx, name, 1)
    last = ctx.classify_reuse()
    assert last["reused"] == after["reused"] and last["classified"] == after["classified"] + Q.FRAME_SLOTS, (after, last)
    MV.build(fresh, case, steps[1][2])
    _same(ctx, fresh, name, "after the kept classifications were dropped", spp=1)


@gpu
def test_a_context_that_never_queues_a_commit_is_unchanged():
    """Two runs of move_tools' multi-leaf sequence with the blocking commit_moved in place: frames, light-space arrays and mesh trees as
    they lie in device memory are the same bytes, and the context holds the scene's own arrays alone."""
    name = "multi-leaf"
    case = S.CASES[name]
    runs = []
    for _ in range(2):
        c = ft.Context(device=0)
        try:
            c.set_option("moved_in_place", 1)
            steps = MV.sequence(name)
            hd = MV.build(c, case, steps[0][2])
            seen = []
            for _, _, pose in steps[1:7]:
                MV.move(c, hd, pose)
                seen.append(MV.render(c, name)[0].tobytes())
                seen += [a.tobytes() for a in light_space(c)]
                trees = c.mesh_trees()
                seen += [trees[k].tobytes() for k in ("nodes", "bsp_leaves", "tris", "wide", "coarse_boxes")]
            assert c.pose_queue() == dict(ZEROS, sets=1)
            runs.append(seen)
        finally:
            c.close()
    assert runs[0] == runs[1]

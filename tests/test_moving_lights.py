"""Moving lights: ft_scene_set_directional / _soft_directional / _positional and ft_scene_commit_lights (include/functracer_hip.h,
DESIGN.md 17) on the shadow cases of tests/shadow_tools.py, through the light sequences of tests/light_tools.py.

The CPU half checks the setters' arithmetic and every documented refusal on a host-only context, that a host-only commit_lights is the
full host commit, and on the oracle alone that every step of every sequence casts shadows in view and changes the frame.

The GPU half walks every sequence with one commit_lights per step and compares, at every step, the frame and the counters with a second
context built from scratch with that step's lights, bit for bit; reads the trees and grids back from device memory and checks that they
hold what they must and are of the kind the step calls for; and checks that revisiting directions reproduces the arrays byte for byte
and at the same sizes.  Then the orderings with queued frames, reused classifications, the temporal accumulation and the other commits."""
import ctypes as C
import os

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd._capi import FtError

from . import helpers as H
from . import light_tools as L
from . import shadow_tools as S
from . import walk_tools as W
from . import test_temporal as T
from .test_light_space_grid import grid_of
from .test_light_space_shadows import NONE, light_space, pair_root

gpu = pytest.mark.gpu
INVALID, STATE = -1, -5


def _status(fn, *args):
    with pytest.raises(FtError) as e:
        fn(*args)
    return e.value.status, str(e.value)


def test_header_declares_and_library_exports_the_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    lib = ft.hip_lib()
    for name in ("ft_scene_set_directional", "ft_scene_set_soft_directional", "ft_scene_set_positional", "ft_scene_commit_lights"):
        assert f"int32_t {name}(ft_context* ctx" in hdr and hasattr(lib, name)
    assert lib.ft_abi_version() == 2 and "#define FT_ABI_VERSION 2" in hdr


# =============================================================================================================================
# CPU half

def _host(name="multi-leaf", lights=None):
    ctx = ft.Context(host_only=True)
    case = S.CASES[name]
    L.build(ctx, case, lights if lights is not None else L.initial(case))
    return ctx


def _held(ctx):
    """What can be read of the scene a context HOLDS while edits are pending (ft_debug_light_space answers for committed scenes only): the
    leaves' matrices of the last successful commit."""
    return [a.tobytes() for a in ctx.leaf_matrices()]


def _state(ctx):
    return [a.tobytes() for a in light_space(ctx)] + [sorted(ctx.scene_info().items())]


def test_setters_refuse_bad_arguments_and_change_nothing():
    ctx = _host()                                                   # lights: soft, point, dir, dir
    before = _state(ctx)
    lib = ctx._lib
    v = (C.c_double * 3)(0.0, -1.0, 0.0)
    assert lib.ft_scene_set_directional(None, 2, v, v) == INVALID
    assert lib.ft_scene_set_directional(ctx._ctx, 2, None, v) == INVALID and lib.ft_scene_set_directional(ctx._ctx, 2, v, None) == INVALID
    assert lib.ft_scene_set_soft_directional(ctx._ctx, 0, None, 0.1, v) == INVALID and lib.ft_scene_set_soft_directional(ctx._ctx, 0, v, 0.1, None) == INVALID
    assert lib.ft_scene_set_positional(ctx._ctx, 1, None, v, v) == INVALID and lib.ft_scene_set_positional(ctx._ctx, 1, v, None, v) == INVALID
    assert lib.ft_scene_set_positional(ctx._ctx, 1, v, v, None) == INVALID
    for fn, args in ((ctx.set_directional, (v, v)), (ctx.set_soft_directional, (v, 0.1, v)), (ctx.set_positional, (v, v, v))):
        for index in (-1, 4, 1 << 20):
            status, text = _status(fn, index, *[tuple(a) if not isinstance(a, float) else a for a in args])
            assert status == INVALID and "no such light" in text
    for fn, index, args in ((ctx.set_directional, 0, ((0, -1, 0), (1, 1, 1))), (ctx.set_directional, 1, ((0, -1, 0), (1, 1, 1))),
                            (ctx.set_soft_directional, 2, ((0, -1, 0), 0.1, (1, 1, 1))), (ctx.set_positional, 3, ((0, 1, 0), (1, 0, 0), (1, 1, 1)))):
        status, text = _status(fn, index, *args)
        assert status == INVALID and "another kind" in text
    ctx.commit_lights()                                             # nothing was changed, nothing is pending: the same scene
    assert _state(ctx) == before
    ctx.close()


def test_setters_use_the_arithmetic_of_the_adders():
    """A plain commit after the setters gives what a fresh graph with those lights gives (the record's frame shows the normalised
    direction; scene_info and every array are equal byte for byte)."""
    case = S.CASES["multi-leaf"]
    steps = L.sequence("multi-leaf")
    for what, lights in (steps[3], steps[6], steps[-2]):
        ctx, fresh = _host(), _host(lights=lights)
        L.set_lights(ctx, lights)
        ctx.commit()
        assert _state(ctx) == _state(fresh), what
        ctx.close()
        fresh.close()


def test_host_only_commit_lights_is_the_full_host_commit():
    for name in ("multi-leaf", "two_clusters", "blob(65)-mirror"):
        ctx = _host(name)
        for what, lights in L.sequence(name)[1:]:
            L.set_lights(ctx, lights)
            ctx.commit_lights()
            fresh = _host(name, lights)
            assert _state(ctx) == _state(fresh), (name, what)
            fresh.close()
        ctx.close()


def test_commit_lights_refuses_what_it_documents():
    """Every FT_ERR_STATE path: its message, and nothing changed - the held scene reads as before, and the full commit that the message
    names then gives what a fresh context with the pending edits gives."""
    case = S.CASES["blob(8)"]
    ctx = ft.Context(host_only=True)
    status, text = _status(ctx.commit_lights)
    assert status == STATE and "no committed scene" in text
    # a structural change
    L.build(ctx, case, L.initial(case))
    before = _state(ctx)
    ctx.add_directional((0, -1, 0), (1, 1, 1))
    held = _held(ctx)
    status, text = _status(ctx.commit_lights)
    assert status == STATE and "ft_scene_commit" in text and "changed since the commit" in text
    assert _held(ctx) == held
    # a pending transform, a pending deformation, a pending commit-time option: each names the call that comes first
    recv_ops, _ = S.geometry(case)
    tris = S.mesh_tris("blob(8)").reshape(-1, 9)

    def build(c, lights, ops, t):
        c.clear()
        mesh = c.bsp_mesh(0, t)
        xf = c.transform(ops, mesh)
        c.set_objects(c.group([c.material(xf, colour=S.MESH_COLOUR), c.material(c.transform(recv_ops, c.primitive(ft.SQUARE)), colour=S.RECEIVER_COLOUR)]))
        L.add_lights(c, lights)
        c.commit()
        return mesh, xf

    def fresh_state(lights, ops, t):
        c = ft.Context(host_only=True)
        build(c, lights, ops, t)
        out = _state(c)
        c.close()
        return out

    lights0 = L.initial(case)
    ops0, ops1 = [("translate", (0.0, 0.0, 0.0))], [("translate", (0.1, 0.0, 0.0))]
    mesh, xf = build(ctx, lights0, ops0, tris)
    before = _state(ctx)
    lights1 = [("dir", (0.0, -1.0, 0.0), (1.0, 1.0, 1.0)), lights0[1]]
    ctx.set_directional(0, lights1[0][1], lights1[0][2])
    ctx.set_transform(xf, ops1)
    held = _held(ctx)
    status, text = _status(ctx.commit_lights)
    assert status == STATE and "ft_scene_commit_moved first" in text
    assert _held(ctx) == held   # the held scene as it was
    ctx.commit_moved()                                              # picks the light up as well
    assert _state(ctx) == fresh_state(lights1, ops1, tris)
    before = _state(ctx)
    bent = tris * 1.01
    ctx.set_mesh_triangles(mesh, bent)
    held = _held(ctx)
    status, text = _status(ctx.commit_lights)
    assert status == STATE and "ft_scene_commit_deformed first" in text
    assert _held(ctx) == held
    ctx.commit_deformed()
    assert _state(ctx) == fresh_state(lights1, ops1, bent)
    before = _state(ctx)
    lights2 = [lights1[0], ("dir", (1.0, -1.0, 0.0), (1.0, 1.0, 1.0))]
    ctx.set_directional(1, lights2[1][1], lights2[1][2])
    held = _held(ctx)
    status, text = _status(ctx.commit_deformed)                     # and the other way round
    assert status == STATE and "ft_scene_commit_lights first" in text
    assert _held(ctx) == held
    ctx.commit_lights()
    assert _state(ctx) == fresh_state(lights2, ops1, bent)
    before = _state(ctx)
    ctx.set_option("light_space_shadows", 1)
    held = _held(ctx)
    status, text = _status(ctx.commit_lights)
    assert status == STATE and "option" in text
    assert _held(ctx) == held
    ctx.set_option("light_space_shadows", 2)
    ctx.commit()
    assert _state(ctx) == before
    ctx.commit_lights()                                             # nothing pending: allowed, and the same scene
    assert _state(ctx) == before
    ctx.close()


@pytest.mark.parametrize("name", L.NAMES)
def test_every_step_casts_shadows_and_changes_the_frame_on_the_oracle(name):
    """A condition on the reference alone: every step but the zero direction leaves at least 20 receiver pixels in view in some
    directional light's shadow, and consecutive steps' frames differ."""
    steps, seen = L.sequence(name), L.oracle_steps(name)
    print(f"{name}: receiver pixels shadowed per step {[(what, n) for (what, _), (n, _) in zip(steps, seen)]}")
    for k, ((what, _), (n, frame)) in enumerate(zip(steps, seen)):
        if what != "zero":
            assert n >= 20, (name, what, n)
        if k:
            assert not np.array_equal(frame, seen[k - 1][1]), (name, what)


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


def _render(c, view, spp, **kw):
    return c.render(W.camera(view), view.w, view.h, spp, S.jitter(spp), tiles=view.tiles, **kw)


def _same(ctx, fresh, view, spp, what):
    a, sa = _render(ctx, view, spp)
    b, sb = _render(fresh, view, spp)
    diff = np.any(a != b, axis=2) & ~(np.isnan(a).all(axis=2) & np.isnan(b).all(axis=2))
    assert not diff.any(), f"{what} x{spp}: {int(diff.sum())} pixels differ from the fresh context, first {np.argwhere(diff)[:3].tolist()}"
    assert L.counters(sa) == L.counters(sb), f"{what} x{spp}"
    assert sa["rays_shadow"] > 0, what
    return a


def _arrays(ctx):
    return [a.tobytes() for a in light_space(ctx)[:3]]


@gpu
@pytest.mark.parametrize("name", L.NAMES)
def test_sequence_matches_a_fresh_context_at_every_step(ctx, fresh, name):
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    steps = L.sequence(name)
    L.build(ctx, case, steps[0][1])
    probe = len(steps) // 2
    kept = {}
    previous = None
    for k, (what, lights) in enumerate(steps[1:], 1):
        L.set_lights(ctx, lights)
        ctx.commit_lights()
        L.build(fresh, case, lights)
        label = f"{name} step {k} ({what})"
        frame = _same(ctx, fresh, view, 1, label)
        _same(ctx, fresh, view, 4, label)
        assert previous is None or not np.array_equal(frame, previous), f"{label}: the frame did not change"
        previous = frame
        kinds, arrays = L.check_structures(ctx, case, lights)
        print(f"{label}: grids {kinds}")
        # (c) the kind of structure the step calls for
        for (part, l), (nu, nv) in kinds.items():
            turned_onto_diagonal = tuple(lights[l][1]) == tuple(S.DIAGONAL)
            if name == "two_clusters":
                assert (nu > 0) == turned_onto_diagonal, label
            elif case.parts[part][0] in S.TREE_ONLY:
                assert nu == 0, label
            else:
                assert nu > 0, label
        if name == "flat-in-plane" and what == "exchanged":         # the in-plane direction on the other light: a grid one cell wide, built on the device
            _, _, nu, nv = grid_of(dict(S.pairs_of(name))[1])       # (what the host builds for that direction)
            assert kinds[(0, 0)] == (nu, nv) and min(nu, nv) == 1 and max(nu, nv) >= 64, (label, kinds)
        if what in ("tilted further", "original again"):
            kept[what] = [a.tobytes() for a in arrays[:3]]
        if k == probe:                                              # the ray queries and the surface buffers, once per case
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
    # (d), (e): A, B, A, B, A - the bytes and the sizes of another visit are those of the first
    a_lights, b_lights = steps[3][1], steps[0][1]
    for turn in range(2):
        L.set_lights(ctx, a_lights)
        ctx.commit_lights()
        assert _arrays(ctx) == kept["tilted further"], f"{name}: visit {turn + 2} of the tilted lights left other bytes"
        L.set_lights(ctx, b_lights)
        ctx.commit_lights()
        assert _arrays(ctx) == kept["original again"], f"{name}: visit {turn + 2} of the original lights left other bytes"


@gpu
def test_a_frame_queued_before_the_call_shows_the_old_lights(ctx, fresh):
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


@gpu
def test_a_reused_classification_does_not_outlive_the_call(ctx, fresh):
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
def test_the_temporal_accumulation_stays_open(ctx):
    """Two accumulates, commit_lights, a third: the history continues (a full commit would have closed it) and the set is the numpy
    restatement's (tests/test_temporal.py) fed with the new lights' frame: the third call counts as call 3 and finds history."""
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
        c, _ = ctx.render(cam, w, h, 1, jit, seed=100 + k)
        frames.append(c)
        p, n, leaf = T._surfaces(ctx, cam, w, h, 1, jit, 0, 100 + k)
        ctx.temporal_accumulate(cam, 1, jit, sample=0, seed=100 + k)
        st = T.reference(st, T.image_plane(cam, w, h), c, p, n, leaf, inside)
        T._compare(ctx, st, inside & ~st["taint"], f"moving lights call {k}")
        status = ctx.temporal_status()
        assert status["calls"] == k + 1
    assert not np.array_equal(frames[2], frames[1])
    assert status["with_history"] > 0 and status["with_history"] >= int(st["history"].sum()) - int(st["taint"].sum())
    ctx.temporal_end()


@gpu
def test_ordering_with_the_other_commits(ctx, fresh):
    case, view = S.CASES["blob(65)-xf"], S.view_of(S.CASES["blob(65)-xf"])
    steps = L.sequence("blob(65)-xf")
    recv_ops, _ = S.geometry(case)
    tris = S.mesh_tris("blob(65)").reshape(-1, 9)

    def build(c, lights, ops, t):
        c.clear()
        mesh = c.bsp_mesh(0, t)
        xf = c.transform(ops, mesh)
        c.set_objects(c.group([c.material(xf, colour=S.MESH_COLOUR), c.material(c.transform(recv_ops, c.primitive(ft.SQUARE)), colour=S.RECEIVER_COLOUR)]))
        L.add_lights(c, lights)
        c.commit()
        return mesh, xf

    ops0, ops1 = list(case.parts[0][1]), list(case.parts[0][1]) + [("translate", (0.05, 0.0, 0.02))]
    mesh, xf = build(ctx, steps[0][1], ops0, tris)
    # a refused call on the device path changes nothing: with the edits taken back the old scene renders as before, bit for bit
    old, old_stats = _render(ctx, view, 1)
    old_arrays = _arrays(ctx)
    L.set_lights(ctx, steps[3][1])
    ctx.set_transform(xf, ops1)
    with pytest.raises(FtError) as e:
        ctx.commit_lights()
    assert e.value.status == STATE and "ft_scene_commit_moved first" in str(e.value)
    L.set_lights(ctx, steps[0][1])
    ctx.set_transform(xf, ops0)
    ctx.commit_moved()
    again, again_stats = _render(ctx, view, 1)
    assert np.array_equal(again, old, equal_nan=True) and L.counters(again_stats) == L.counters(old_stats) and _arrays(ctx) == old_arrays
    # commit_moved after a pending setter picks the lights up
    L.set_lights(ctx, steps[2][1])
    ctx.set_transform(xf, ops1)
    with pytest.raises(FtError) as e:
        ctx.commit_lights()
    assert e.value.status == STATE and "ft_scene_commit_moved first" in str(e.value)
    ctx.commit_moved()
    build(fresh, steps[2][1], ops1, tris)
    _same(ctx, fresh, view, 1, "commit_moved with a pending setter")
    # commit_deformed with a pending setter is refused; after it the edited mesh stays without pairs through commit_lights
    bent = tris * np.array([1.0, 1.02, 1.0] * 3)
    ctx.set_mesh_triangles(mesh, bent)
    ctx.set_directional(0, steps[3][1][0][1], steps[3][1][0][2])
    with pytest.raises(FtError) as e:
        ctx.commit_deformed()
    assert e.value.status == STATE and "ft_scene_commit_lights first" in str(e.value)
    with pytest.raises(FtError) as e:
        ctx.commit_lights()
    assert e.value.status == STATE and "ft_scene_commit_deformed first" in str(e.value)
    L.set_lights(ctx, steps[2][1])                                  # back to the committed lights: commit_moved's
    ctx.commit()                                                    # (a full commit clears every pending edit)
    ctx.set_mesh_triangles(mesh, bent * 1.0)
    ctx.commit_deformed()
    assert light_space(ctx)[3][0] == 0xFFFFFFFF
    L.set_lights(ctx, steps[3][1])
    ctx.commit_lights()
    assert light_space(ctx)[3][0] == 0xFFFFFFFF
    build(fresh, steps[3][1], ops1, bent)
    _same(ctx, fresh, view, 1, "commit_lights after commit_deformed")
    _same(ctx, fresh, view, 4, "commit_lights after commit_deformed")


@gpu
@pytest.mark.parametrize("option", (0, 1))
def test_options_without_grids(option):
    ctx, fresh = ft.Context(device=0), ft.Context(device=0)
    try:
        for c in (ctx, fresh):
            c.set_option("light_space_shadows", option)
        for name in ("blob(65)-mirror", "multi-leaf"):
            case, view = S.CASES[name], S.view_of(S.CASES[name])
            steps = L.sequence(name)
            L.build(ctx, case, steps[0][1])
            sizes = [len(a) for a in light_space(ctx)[:3]]
            for k, (what, lights) in enumerate(steps[1:], 1):
                L.set_lights(ctx, lights)
                ctx.commit_lights()
                L.build(fresh, case, lights)
                _same(ctx, fresh, view, 1, f"option {option} {name} step {k}")
                pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
                assert [len(pairs), len(nodes), len(ls_tris)] == sizes
                if option == 0:
                    assert (leaf_pairs == 0xFFFFFFFF).all()
                else:
                    kinds, _ = L.check_structures(ctx, case, lights, grids=False)
                    assert kinds and all(nu == 0 for nu, _ in kinds.values())
    finally:
        ctx.close()
        fresh.close()


def _two_devices(ctx, fresh):
    ordinals = ctx.devices()
    try:
        name = "multi-leaf"
        case, view = S.CASES[name], S.view_of(S.CASES[name])
        steps = L.sequence(name)
        L.build(ctx, case, steps[0][1])
        for k, (what, lights) in enumerate(steps[1:], 1):
            L.set_lights(ctx, lights)
            ctx.commit_lights()
            L.build(fresh, case, lights)
            for spp in (1, 4):
                a, sa = _render(ctx, view, spp)
                b, _ = _render(fresh, view, spp)
                assert np.array_equal(a, b, equal_nan=True), f"{ordinals} step {k} ({what}) x{spp}"
                assert sa["rays_shadow"] > 0
            L.check_structures(ctx, case, lights)
    finally:
        ctx.close()


@gpu
def test_two_devices(fresh):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _two_devices(ft.Context(device=[0, 1]), fresh)


@gpu
def test_two_device_context_on_one_gpu(fresh):
    _two_devices(ft.Context(device=[0, 0]), fresh)

"""ft_temporal_enqueue / ft_temporal_wait (Context.temporal_enqueue / temporal_wait): ft_temporal_accumulate and the ft_temporal_filter of
its result as one queued call behind the frames of ft_render_enqueue (include/functracer_hip.h).

The rule every device test here checks: a queued call produces, bit for bit, what the blocking pair produces.  So each test runs the
blocking sequence first, then ft_temporal_begin again and the queued sequence on the same session context, and compares with
np.array_equal - the two run the same kernels on the same inputs, and a tolerance would hide exactly the ordering faults the tests are for.
The sizes are those of tests/test_temporal.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from functracer_amd._capi import FtError

from . import helpers as H
from .test_temporal import TILES, W, Hh, _camera, _load, _rot_y, orbit
from .test_temporal_motion import _bunny_tris, _pose
from .test_temporal_motion import _camera as motion_camera

DEPTH = 4                                                            # FT_TEMPORAL_QUEUE_DEPTH
REGION = TILES + [(-4, 30, 12, 9)]                                   # the three tiles (the third is cut by the frame's corner) and a rect cut by its left edge
FORMS = {"accumulate": None, "filter": dict(demodulate=0), "filter+demodulate": dict(demodulate=1)}
FOLLOW = "temporal_follow_deformed"


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_the_queued_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"#define FT_TEMPORAL_QUEUE_DEPTH 4\b", hdr) and _capi.TEMPORAL_QUEUE_DEPTH == DEPTH
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t ft_temporal_enqueue\(ft_context\* ctx, const ft_camera\* cam, int32_t spp, const double\* jitter_xy, int32_t sample, uint64_t seed,\s*"
                     r"const ft_temporal_params\* params, const ft_temporal_filter_params\* filter\s*,\s*int32_t rgba8, void\* host_out\);", flat)
    assert re.search(r"int32_t ft_temporal_wait\(ft_context\* ctx, ft_stats\* stats\);", flat)
    assert "#define FT_ABI_VERSION 2" in hdr
    lib = C.CDLL(ft.HIP_LIB)
    for name in ("ft_temporal_enqueue", "ft_temporal_wait"):
        assert hasattr(lib, name), name


def _raw_enqueue(ctx, cam, jit, spp=4, sample=0, rgba8=0, out=None, filt=None, null_cam=False, null_params=False, null_jitter=False, **kw):
    """ft_temporal_enqueue itself, past the Python layer's own checks.  kw: fields of ft_temporal_params; filt: None or fields of
    ft_temporal_filter_params."""
    p = _capi.ft_temporal_params()
    for k, v in {**_capi.TEMPORAL_DEFAULTS, **kw}.items():
        setattr(p, k, v)
    fp = None
    if filt is not None:
        fp = _capi.ft_temporal_filter_params()
        for k, v in {**_capi.TEMPORAL_FILTER_DEFAULTS, **filt}.items():
            setattr(fp, k, v)
    return ft.hip_lib().ft_temporal_enqueue(ctx._ctx, None if null_cam else C.byref(cam), spp, None if null_jitter else _capi.dptr(jit), sample, 1,
                                            None if null_params else C.byref(p), C.byref(fp) if fp is not None else None, rgba8,
                                            out.ctypes.data_as(C.c_void_p) if out is not None else None)


def test_arguments_are_checked_in_order_before_the_device():
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    cam = ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 16 / 9)
    jit, out = np.zeros((4, 2)), np.zeros((18, 32, 3))

    def call(**kw):
        return _raw_enqueue(ctx, cam, jit, **kw)

    # ft_temporal_accumulate's checks, in its order
    assert call(spp=0) == -4 and call(spp=0, sample=9, max_history=0, null_cam=True, to_frame=1) == -4
    assert call(sample=4) == -1 and call(sample=-1) == -1 and call(spp=-1) == -1 and call(null_jitter=True) == -1
    assert call(null_cam=True) == -1 and call(null_params=True) == -1
    assert call(max_history=0) == -1 and call(min_normal_dot=float("nan")) == -1 and call(min_normal_dot=1.5) == -1
    assert call(position_tolerance_px=0.0) == -1 and call(position_tolerance_px=float("nan")) == -1
    # then the filter's: a filter needs somewhere to put its result, then ft_temporal_filter's checks in its order
    assert call(filt={}) == -1 and call(filt={}, out=None, max_history=0) == -1
    assert call(filt=dict(iterations=7), out=out) == -1 and call(filt=dict(iterations=-1), out=out) == -1
    assert call(filt=dict(sigma_colour=-1.0), out=out) == -1 and call(filt=dict(sigma_normal=float("nan")), out=out) == -1
    assert call(filt=dict(min_history=0), out=out) == -1 and call(filt=dict(variance_floor=0.0), out=out) == -1
    assert call(filt=dict(demodulate=1, albedo_floor=0.0), out=out) == -1 and call(filt=dict(demodulate=0, albedo_floor=0.0), out=out) == -2
    # then what the queued call does not offer, the accumulate's before the filter's, each naming the blocking call
    assert call(to_frame=1) == -1 and "ft_temporal_accumulate" in ctx.last_error()
    assert call(to_frame=1, filt=dict(to_frame=1), out=out) == -1 and "ft_temporal_accumulate" in ctx.last_error()
    assert call(filt=dict(to_frame=1), out=out) == -1 and "ft_temporal_filter" in ctx.last_error()
    assert call(filt=dict(to_frame=1, iterations=9), out=out) == -1 and "iterations" in ctx.last_error()   # an argument error comes first
    # valid: a host-only context has no device, and that is said before the missing begin (FT_ERR_STATE) could be
    assert call() == -2 and call(out=out) == -2 and call(filt={}, out=out) == -2 and call(filt=dict(demodulate=0, iterations=0), out=out, rgba8=1) == -2
    assert ft.hip_lib().ft_temporal_wait(ctx._ctx, None) == -2 and ft.hip_lib().ft_temporal_wait(None, None) == -1
    with pytest.raises(FtError) as e:                                # the Python layer sizes its output by the begin
        ctx.temporal_enqueue(cam, 1, jit[:1])
    assert e.value.status == -5
    with pytest.raises(ValueError):
        ctx.temporal_enqueue(cam, 1, jit[:1], history=3)
    with pytest.raises(ValueError):
        ctx._temporal = (32, 18)
        ctx.temporal_enqueue(cam, 1, jit[:1], filter=dict(passes=3))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
@pytest.fixture(scope="module")
def rings():
    """Page-locked result buffers, made once: rings(shape, dtype, n) -> n arrays."""
    made = {}

    def get(shape, dtype, n=DEPTH):
        key = (tuple(shape), np.dtype(dtype).str)
        have = made.setdefault(key, [])
        while len(have) < n:
            have.append(ft.PinnedArray(shape, dtype))
        return [p.array for p in have[:n]]

    yield get
    for ps in made.values():
        for p in ps:
            p.close()


def _shape(rgba8, w=W, h=Hh):
    return ((h, w, 4), np.uint8) if rgba8 else ((h, w, 3), np.float64)


def _final(ctx):
    """What is compared after the last call: ft_temporal_fetch's planes and the two status calls."""
    M, se, N = ctx.temporal_fetch()
    return dict(M=M, se=se, N=N, status=ctx.temporal_status(), clamp=ctx.temporal_clamp_status())


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(a, b, equal_nan=(a.dtype != np.uint8)), f"{what}: {int((a != b).sum())} values differ"


def _same_final(got, want, what):
    for k in ("M", "se", "N"):
        _same(got[k], want[k], f"{what}: ft_temporal_fetch {k}")
    assert got["status"] == want["status"], f"{what}: {got['status']} != {want['status']}"
    assert got["clamp"] == want["clamp"], f"{what}: {got['clamp']} != {want['clamp']}"


def _blocking(ctx, cams, spp, jit, region, filt, rgba8, clamp=None, w=W, h=Hh, seed0=100, between=None, render=None):
    """The blocking sequence: per camera a frame, ft_temporal_accumulate and - with a filter - ft_temporal_filter.  Returns the results of
    the calls, the final state, and the launches of the last call (the pair's, and the k_aov launches of the filter's guide pass).
    between(k): run in front of call k (commits, other calls); render(k, cam): replaces the blocking ft_render."""
    shape, dtype = _shape(rgba8, w, h)
    sample = spp - 1
    ctx.temporal_begin(w, h, tiles=region)
    if clamp:
        ctx.temporal_set_clamp(radius=clamp)
    outs, launches = [], None
    for k, cam in enumerate(cams):
        if between:
            between(k)
        if render:
            render(k, cam)
        else:
            ctx.render(cam, w, h, spp, jit, seed=seed0 + k, fetch=False)
        out = np.full(shape, 7, dtype=dtype)
        if filt is None:
            _, st = ctx.temporal_accumulate(cam, spp, jit, sample=sample, seed=seed0 + k, rgba8=rgba8, out=out)
            launches = (st["n_launches"], 0, st["hits_primary"])
        else:
            _, st = ctx.temporal_accumulate(cam, spp, jit, sample=sample, seed=seed0 + k, fetch=False)
            _, _, sf = ctx.temporal_filter(cam, spp, jit, sample=sample, seed=seed0 + k, rgba8=rgba8, out=out, **filt)
            n_pix = ctx.temporal_status()["pixels"]
            per = max(1, min(n_pix, ctx_chunk(ctx)))
            per -= per % 64 if per > 64 else 0
            launches = (st["n_launches"] + sf["n_launches"], math.ceil(n_pix / per) if filt.get("demodulate", 1) and n_pix else 0, st["hits_primary"])
        outs.append(out)
    return outs, _final(ctx), launches


_CHUNK = {}


def ctx_chunk(ctx):
    """The "chunk_samples" the tests of this module have set on `ctx` (the option cannot be read back)."""
    return _CHUNK.get(id(ctx), 16 << 20)


def _queued(ctx, cams, spp, jit, region, filt, rgba8, ring, clamp=None, w=W, h=Hh, seed0=100, between=None, render=None, want=None, what=""):
    """The same sequence queued: ft_render_enqueue and ft_temporal_enqueue per camera, the results into the ring's page-locked buffers
    round-robin.  The host waits only where it must: before a buffer is handed to call k + len(ring), and at the end.  want: the blocking
    sequence's results, compared as soon as a wait has made a buffer the host's again.  Returns the final state and the last call's stats."""
    sample = spp - 1
    ctx.temporal_begin(w, h, tiles=region)
    if clamp:
        ctx.temporal_set_clamp(radius=clamp)
    checked, stats = 0, None

    def check(upto):
        nonlocal checked
        for j in range(checked, upto):
            _same(ring[j % len(ring)], want[j], f"{what}: host_out of call {j}")
        checked = upto

    for k, cam in enumerate(cams):
        if between and between(k):                                  # (true: it retired the queue)
            check(k)
        if k - checked >= len(ring):
            stats = ctx.temporal_wait()
            check(k)
        if render:
            render(k, cam)
        else:
            ctx.render_enqueue(cam, w, h, spp, jit, seed=seed0 + k)
        out = ring[k % len(ring)]
        out[...] = 7
        ctx.temporal_enqueue(cam, spp, jit, sample=sample, seed=seed0 + k, rgba8=rgba8, out=out, filter=filt)
    stats = ctx.temporal_wait()
    check(len(cams))
    assert ctx.temporal_wait()["n_launches"] == 0                  # nothing queued: FT_OK, zeroed stats
    return _final(ctx), stats


# ---------------------------------------------------------------------------------------------------------------- 1. queued equals blocking
@pytest.mark.gpu
@pytest.mark.parametrize("region", [None, REGION], ids=["frame", "tiles"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("name", ["bunny", "hollow-sphere", "sample-soft"])
def test_queued_equals_blocking(hip, rings, name, spp, region):
    """Six calls along the orbit in every form - no filter, filter, filter with demodulate, each as FP64 and RGBA8 - with the clamp off and
    on at r = 2.  The demodulate form runs one guide pass where the blocking pair runs two."""
    scene = _load(hip, name)
    cams = orbit(scene.camera, 6)
    jit = ft.jitter_pattern(spp)
    hip.render(cams[0], W, Hh, spp, jit, fetch=False)               # (hollow-sphere: a blocking render first, so that its hit lists have grown)
    for form, filt in FORMS.items():
        for rgba8 in (False, True):
            for clamp in (None, 2):
                what = f"{name} x{spp} {'tiles' if region else 'frame'} {form} {'rgba8' if rgba8 else 'fp64'} clamp {clamp}"
                outs, final, launches = _blocking(hip, cams, spp, jit, region, filt, rgba8, clamp)
                got, stats = _queued(hip, cams, spp, jit, region, filt, rgba8, rings(*_shape(rgba8)), clamp, want=outs, what=what)
                _same_final(got, final, what)
                assert final["status"]["calls"] == 6 and (clamp is None) == (final["clamp"]["radius"] == 0)
                assert stats["n_launches"] == launches[0] - launches[1], f"{what}: {stats['n_launches']} launches, the blocking pair {launches}"
                assert stats["rays_primary"] == final["status"]["pixels"] and stats["hits_primary"] == launches[2]
                assert stats["trace_kernel_ms"] == 0.0 and stats["kernel_ms"] > 0.0 and stats["wall_ms"] > 0.0
                if form == "filter+demodulate":
                    assert launches[1] >= 1                         # the shared guide pass is the point of this form
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 2. several windows
@pytest.mark.gpu
def test_several_windows_and_a_tiny_frame(hip, rings):
    """chunk_samples 4096 cuts the 14 400 pixels into four windows with nothing but stream order between them; and a 5 x 3 frame under the
    widest clamp, where every neighbourhood and every tap leaves the frame."""
    scene = _load(hip, "bunny")
    cams = orbit(scene.camera, 6)
    jit = ft.jitter_pattern(4)
    try:
        hip.set_option("chunk_samples", 4096)
        _CHUNK[id(hip)] = 4096
        for form, filt in FORMS.items():
            for clamp in (None, 2):
                what = f"four windows {form} clamp {clamp}"
                outs, final, launches = _blocking(hip, cams, 4, jit, None, filt, False, clamp)
                got, stats = _queued(hip, cams, 4, jit, None, filt, False, rings(*_shape(False)), clamp, want=outs, what=what)
                _same_final(got, final, what)
                assert launches[1] == (4 if form == "filter+demodulate" else 0)
                assert stats["n_launches"] == launches[0] - launches[1]
    finally:
        hip.set_option("chunk_samples", 16 << 20)
        _CHUNK.pop(id(hip), None)
    for form, filt in FORMS.items():
        what = f"5 x 3 {form} r = 3"
        outs, final, _ = _blocking(hip, cams, 4, jit, None, filt, False, 3, w=5, h=3)
        got, _ = _queued(hip, cams, 4, jit, None, filt, False, rings((3, 5, 3), np.float64), 3, w=5, h=3, want=outs, what=what)
        _same_final(got, final, what)
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 3. more calls than slots
@pytest.mark.gpu
def test_more_calls_than_slots(hip, rings):
    """Nine calls queued with no wait into four host buffers round-robin: buffers k and k + 4 are the same memory, and call k + 4 waits for
    call k on the host.  Right after call k + 4 was queued - before it reads anything else - the test reads buffer k.  Call k has finished
    by then (that is the rule under test); the copy of call k + 4 into the same memory may or may not have begun, so every pixel must hold
    call k's or call k + 4's value and nothing older: a read that could only pass on call k's bytes would depend on how fast the device is."""
    scene = _load(hip, "bunny")
    cams = orbit(scene.camera, 9)
    jit = ft.jitter_pattern(1)
    filt = dict(demodulate=1)
    outs, final, _ = _blocking(hip, cams, 1, jit, None, filt, True)
    assert not any(np.array_equal(outs[k], outs[k + DEPTH]) for k in range(9 - DEPTH))   # the calls can be told apart
    ring = rings(*_shape(True))
    for r in ring:
        r[...] = 7
    hip.temporal_begin(W, Hh)
    for k, cam in enumerate(cams):
        hip.render_enqueue(cam, W, Hh, 1, jit, seed=100 + k)
        hip.temporal_enqueue(cam, 1, jit, seed=100 + k, rgba8=True, out=ring[k % DEPTH], filter=filt)
        if k >= DEPTH:
            seen = ring[k % DEPTH].copy()
            ok = (seen == outs[k - DEPTH]).all(-1) | (seen == outs[k]).all(-1)
            assert ok.all(), f"buffer {k % DEPTH} after call {k} was queued: {int((~ok).sum())} pixels hold neither call {k - DEPTH}'s nor call {k}'s bytes"
    stats = hip.temporal_wait()
    for k in range(9 - DEPTH, 9):
        _same(ring[k % DEPTH], outs[k], f"host_out of call {k} after the wait")
    _same_final(_final(hip), final, "nine calls, four buffers")
    assert stats["rays_primary"] == W * Hh and stats["wall_ms"] > 0.0
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 4. each call reads its own frame
@pytest.mark.gpu
@pytest.mark.parametrize("mains", [1, 2, 3])
def test_each_call_reads_its_own_frame(hip, mains):
    """render_enqueue, temporal_enqueue, render_enqueue, ... with one wait at the end, the camera alternating between two opposite views of
    night-house so that consecutive frames share almost no pixel: a call that read the frame before its last kernel wrote it, or after the
    next frame's began to, shows another picture.  Every call has a buffer of its own.  This guards the frame's read-before-overwrite order
    on the streams the frame driver uses under "mains" 1, 2 and 3; it is a guard, not a proof - a wrong order can still come out right on
    a fast device.  The argument is the table of DESIGN.md 12.2."""
    w, h, n = 640, 360, 12
    scene = _load(hip, "night-house", pinhole=True)
    cam = scene.camera
    o, look = np.array(cam.o[:]), np.array(cam.look_at[:])
    views = [cam, _camera(look + _rot_y(o - look, 180.0), look, cam)]
    cams = [views[k & 1] for k in range(n)]
    jit = ft.jitter_pattern(1)
    bufs = [ft.PinnedArray((h, w, 4), np.uint8) for _ in range(n)]
    try:
        hip.set_option("mains", mains)
        outs, final, _ = _blocking(hip, cams, 1, jit, None, None, True, w=w, h=h)
        assert not np.array_equal(outs[-1], outs[-2])
        got, _ = _queued(hip, cams, 1, jit, None, None, True, [b.array for b in bufs], w=w, h=h, want=outs, what=f"mains {mains}")
        _same_final(got, final, f"mains {mains}")
    finally:
        hip.set_option("mains", 2)
        hip.temporal_end()
        hip.wait()
        for b in bufs:
            b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. moving and deforming
def _build_motion_scene(ctx, pose):
    """The hand-built scene of tests/test_temporal_motion.py (_build), with the handle of its mesh node as well."""
    ctx.clear()
    hd = {}
    ground = ctx.material(ctx.primitive(ft.PLANE), colour=(0.6, 0.6, 0.55))
    hd["sphere"] = ctx.transform(pose["sphere"], ctx.primitive(ft.SPHERE))
    sphere = ctx.material(hd["sphere"], colour=(0.9, 0.3, 0.2), apply_lighting=False)
    hd["cube"] = ctx.transform(pose["cube"], ctx.primitive(ft.CUBE))
    cube = ctx.material(hd["cube"], colour=(0.2, 0.5, 0.9), shineyness=8.0)
    bunny = ctx.bsp_mesh(0, _bunny_tris())
    hd["mesh"] = ctx.transform(pose["mesh"], bunny)
    mesh = ctx.material(hd["mesh"], colour=(0.8, 0.8, 0.3))
    hd["operand"] = ctx.transform(pose["operand"], ctx.primitive(ft.SPHERE))
    block = ctx.transform([("scale", 1.4), ("translate", (1.8, 0.7, 0.0))], ctx.primitive(ft.CUBE))
    csg = ctx.material(ctx.subtract(block, hd["operand"]), colour=(0.3, 0.8, 0.4))
    ctx.set_objects(ctx.group([ground, sphere, cube, mesh, csg]))
    ctx.add_directional((0.4, -1.0, 0.6), (1.0, 1.0, 1.0))
    ctx.commit()
    return hd, bunny


@pytest.mark.gpu
def test_moving_and_deforming_between_queued_calls(hip, rings):
    """A commit_moved in front of call 2 and a commit_deformed under "temporal_follow_deformed" in front of call 4: the commits retire the
    queue, the call behind each follows the leaves / the triangles as the blocking call does, and its records outlive the enqueue."""
    cams = orbit(motion_camera(), 6)
    jit = ft.jitter_pattern(4)
    bent = np.asarray(_bunny_tris()).reshape(-1, 9).copy()
    bent[:, 1::3] *= 1.04                                           # every vertex a little higher: every triangle of the mesh changes

    def sequence(run, **kw):
        hd, bunny = _build_motion_scene(hip, _pose(0.0))
        hip.render(cams[0], W, Hh, 4, jit, fetch=False)             # (the CSG operand: grown lists before anything is queued)

        def between(k):
            if k == 2:
                for name, ops in _pose(2.0).items():
                    hip.set_transform(hd[name], ops)
                hip.commit_moved()
            elif k == 4:
                hip.set_mesh_triangles(bunny, bent)
                hip.commit_deformed()
            return k in (2, 4)
        return run(hip, cams, 4, jit, None, dict(demodulate=1), False, between=between, **kw)

    try:
        hip.set_option(FOLLOW, 1)
        outs, final, _ = sequence(_blocking)
        got, _ = sequence(_queued, ring=rings(*_shape(False)), want=outs, what="moved and deformed")
        _same_final(got, final, "moved and deformed")
        assert final["status"]["with_history"] > 0
    finally:
        hip.set_option(FOLLOW, 0)
        hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 6. errors leave no trace
@pytest.mark.gpu
def test_refused_calls_leave_no_trace(hip, rings):
    scene = _load(hip, "bunny")
    cams = orbit(scene.camera, 4)
    jit = ft.jitter_pattern(4)
    ring = rings(*_shape(False))
    hip.temporal_end()
    assert _raw_enqueue(hip, cams[0], jit, out=ring[0]) == -5       # no begin
    outs, final, _ = _blocking(hip, cams, 4, jit, REGION, dict(demodulate=1), False)

    def refused(k):
        if k == 1:                                                  # the frame in HBM is RGBA8: refused, and the FP64 frame queued next is read
            hip.render_rgba8(cams[1], W, Hh, 4, jit, fetch=False)
            assert _raw_enqueue(hip, cams[1], jit, out=ring[1], sample=3) == -5
        if k == 2:                                                  # what the queued call does not offer, and a bad argument
            assert _raw_enqueue(hip, cams[2], jit, out=ring[2], to_frame=1) == -1
            assert _raw_enqueue(hip, cams[2], jit, out=ring[2], filt=dict(to_frame=1)) == -1
            assert _raw_enqueue(hip, cams[2], jit, filt={}) == -1 and _raw_enqueue(hip, cams[2], jit, sample=4) == -1
        return False

    got, _ = _queued(hip, cams, 4, jit, REGION, dict(demodulate=1), False, ring, between=refused, want=outs, what="refused calls in between")
    _same_final(got, final, "refused calls in between")
    hip.temporal_end()
    two = ft.Context(device=[0, 0])                                 # several devices: refused as the blocking calls are
    try:
        assert _raw_enqueue(two, cams[0], jit, out=ring[0]) == -4
        assert ft.hip_lib().ft_temporal_wait(two._ctx, None) == 0
    finally:
        two.close()


# ---------------------------------------------------------------------------------------------------------------- 7. overflow
@pytest.mark.gpu
def test_an_overflowing_queued_call_ends_the_accumulation(hip, rings):
    """The mesh under a subtract of test_overflowing_hit_lists_grow_and_the_frame_still_matches at a capacity of 2 hits.  The guide pass of
    a queued call overflows: nothing grows behind the host's back, ft_temporal_wait says so and the accumulation is over.  One blocking
    call grows the lists, which stay, and the queued sequence then equals the blocking one."""
    tris = np.asarray(_bunny_tris()).reshape(-1, 9)
    cam = ft.make_camera((0, 1, -6), (0, 0.6, 0), (0, 1, 0), H.deg(40.0), 1.5)
    cams = orbit(cam, 4)
    jit = np.zeros((1, 2))                                          # (the view, size and pattern of tests/test_aov.py's overflow test: a few primaries cross the mesh more than twice)
    w, h = 96, 64

    def build():
        hip.clear()
        m = hip.scale(7.0, hip.bsp_mesh(3, tris))
        node = hip.subtract(m, hip.translate((0.0, 0.9, -0.3), hip.scale(0.5, hip.primitive(ft.SPHERE))))
        hip.set_objects(hip.group([hip.material(node, colour=(0.8, 0.5, 0.3), reflectance=0.2, shineyness=10)]))
        hip.add_directional((-1, -1, 1), (1, 1, 1))
        hip.commit()

    ring = rings((h, w, 3), np.float64)
    try:
        hip.set_option("csg_mesh_capacity", 2)
        build()
        small = hip.scene_info()["csg_capacity"]
        hip.render(cams[0], w, h, 1, jit, fetch=False)              # grows, so that a frame exists ...
        assert hip.scene_info()["csg_capacity"] > small
        hip.set_option("csg_mesh_capacity", 2)                      # ... and back to lists the guide pass overflows
        build()
        assert hip.scene_info()["csg_capacity"] == small
        hip.set_option("csg_auto_grow", 0)                          # the premise: the guide pass of this view overflows lists of 2 hits
        with pytest.raises(FtError, match="OVERFLOW"):
            hip.render_aov(cams[0], w, h, 1, jit, channels=["leaf"])
        hip.set_option("csg_auto_grow", 1)
        hip.temporal_begin(w, h)
        hip.temporal_enqueue(cams[0], 1, jit, out=ring[0])
        hip.temporal_enqueue(cams[0], 1, jit, out=ring[1])          # (read a history written from overflowed rays)
        with pytest.raises(FtError, match="OVERFLOW"):
            hip.temporal_wait()
        with pytest.raises(FtError, match="STATE"):
            hip.temporal_status()
        assert hip.scene_info()["csg_capacity"] == small            # the lists did not grow
        assert hip.temporal_wait()["n_launches"] == 0               # and nothing is queued any more
        hip.temporal_begin(w, h)                                    # the remedy the header names: one blocking call, whose grown lists stay
        hip.temporal_accumulate(cams[0], 1, jit, fetch=False)
        assert hip.scene_info()["csg_capacity"] > small
        outs, final, _ = _blocking(hip, cams, 1, jit, None, dict(demodulate=1), False, w=w, h=h)
        got, _ = _queued(hip, cams, 1, jit, None, dict(demodulate=1), False, ring, w=w, h=h, want=outs, what="after the lists grew")
        _same_final(got, final, "after the lists grew")
    finally:
        hip.set_option("csg_auto_grow", 1)
        hip.set_option("csg_mesh_capacity", 32)
        hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 8. other calls in between
@pytest.mark.gpu
def test_an_aov_or_denoise_call_between_queued_calls(hip, rings):
    """ft_render_aov (over other tiles, with another pattern) in front of call 2 and ft_denoise in front of call 3: both retire the queue
    and overwrite ft_render_aov's pixel list, jitter pattern and counters; the accumulation's own list survives them."""
    scene = _load(hip, "sample-soft")
    cams = orbit(scene.camera, 5)
    jit = ft.jitter_pattern(4)
    other = ft.jitter_pattern(2)

    def sequence(run, queued=False, **kw):
        def render(k, cam):
            if queued:
                hip.render_enqueue(cam, W, Hh, 4, jit, seed=100 + k)
            else:
                hip.render(cam, W, Hh, 4, jit, seed=100 + k, fetch=False)
            if k == 2:
                hip.render_aov(cam, W, Hh, 2, other, sample=1, seed=5, tiles=[(16, 8, 40, 24)], channels=["p", "leaf"])
            elif k == 3:
                hip.denoise(cam, W, Hh, 2, other, sample=0, seed=9, tiles=[(0, 0, 64, 64)])
        return run(hip, cams, 4, jit, REGION, dict(demodulate=1), False, render=render, **kw)

    outs, final, _ = sequence(_blocking)
    got, _ = sequence(_queued, queued=True, ring=rings(*_shape(False)), want=outs, what="aov and denoise in between")
    _same_final(got, final, "aov and denoise in between")
    hip.temporal_end()

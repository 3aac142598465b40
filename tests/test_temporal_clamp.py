"""ft_temporal_set_clamp / ft_temporal_clamp_status (Context.temporal_set_clamp / temporal_clamp_status): the neighbourhood clamp of the
temporal history, clause 3a of ft_temporal_accumulate (include/functracer_hip.h).  `reference_clamped` restates clauses 1
to 6 with 3a in numpy; with the clamp off it is test_temporal.py's `reference`, bit for bit.  Its inputs come from the public API
(render, render_aov, leaf_matrices), so it shares no code with k_temporal or k_temporal_box.

Beside the taint of `reference` (a tap's compared quantity within NEAR of its threshold, or descent from such a pixel) a pixel is tainted
where a channel of the fetched mean M_h lies within NEAR (relative to the larger of |lo| and |hi|) of lo or hi: there a correct
implementation may or may not count the pixel as clamped, and N differs by more than rounding between the two.

The GPU tests print the figures they assert on; what an MI355X gave is in DESIGN.md 12.1 "Measured"."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import helpers as H
from .test_mesh_refit import Recorder
from .test_temporal import (ATOL, LEFT_OUT_CAP, MIN_WEIGHT, NEAR, RTOL, TILES, _compare, _dot, _flat_inputs, _load, _mask, _surfaces, image_plane,
                            new_state, orbit, project, reference)
from .test_temporal_deform import OPTION as FOLLOW_OPTION
from .test_temporal_deform import _aov, _deformed, _mesh_leaf, _shape, sliver_pixels, taken_back_deformed
from .test_temporal_motion import _build, _grown, _matrices, _pose, motion, taken_back
from .test_temporal_motion import _camera as _motion_camera

W, Hh = 160, 90
CLIPPED = TILES + [(-5, 60, 30, 12)]                                 # test_temporal.TILES and one rect clipped by the frame
AGGRESSIVE = dict(radius=1, clamped_history=1, gamma=1.0, floor=1e-4)   # the setting for noise-free frames; _capi.TEMPORAL_CLAMP_DEFAULTS


# ---------------------------------------------------------------------------------------------------------------- the definition, in numpy
def neighbourhood_box(c, in_tiles, radius, gamma, floor):
    """Clause 3a's box: (lo, hi, k) per pixel of the frame c [h, w, 3].  Taps dy = -r .. r outer, dx = -r .. r inner; a tap takes part iff
    it lies in the frame, is in T and is finite in every channel.  (A tap that does not take part adds 0.0, which changes no bit of a sum
    that started at 0.0.)"""
    h, w = in_tiles.shape
    r = int(radius)
    part = in_tiles & np.isfinite(c).all(-1)
    cz = np.where(part[..., None], c, 0.0)
    pp = np.zeros((h + 2 * r, w + 2 * r), dtype=bool)
    pc = np.zeros((h + 2 * r, w + 2 * r, 3))
    pp[r:r + h, r:r + w], pc[r:r + h, r:r + w] = part, cz
    k, s1, s2 = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            q = pc[dy:dy + h, dx:dx + w]
            k = k + np.where(pp[dy:dy + h, dx:dx + w], 1.0, 0.0)
            s1 = s1 + q
            s2 = s2 + q * q
    with np.errstate(all="ignore"):
        mu = s1 / k[..., None]
        v = s2 / k[..., None] - mu * mu
        sd = np.sqrt(np.where(v > 0.0, v, 0.0))
        hw = gamma * sd + floor
    return mu - hw, mu + hw, k


def reference_clamped(prev, plane, c, p, n, leaf, in_tiles, clamp=None, max_history=32, min_normal_dot=0.9, position_tolerance_px=4.0):
    """One ft_temporal_accumulate, clauses 1 to 6 with 3a: the state after it.  clamp: None (off) or a dict of radius, clamped_history,
    gamma, floor.  Arguments and state as test_temporal.reference; the state also carries `clamped`, the tile pixels with clamped(x)."""
    h, w = leaf.shape
    hit = leaf >= 0
    Wsum, Nh = np.zeros((h, w)), np.zeros((h, w))
    Mh, Qh = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    near, inherited = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    clamped = np.zeros((h, w), dtype=bool)
    with np.errstate(all="ignore"):
        if prev["plane"] is not None:
            pp = prev["plane"]
            fx, fy, zc = project(pp, p)
            ok = hit & (zc > 0.0) & (fx >= -1.0) & (fx < w) & (fy >= -1.0) & (fy < h)
            fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
            x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
            wx, wy = fx - np.floor(fx), fy - np.floor(fy)
            tol2 = (position_tolerance_px * max(pp["pw"], pp["ph"]) * zc) ** 2
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = x0 + dx, y0 + dy
                    inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    cand = inside & (prev["N"][cy, cx] >= 1.0) & (prev["leaf"][cy, cx] == leaf)
                    ndot = _dot(n, prev["n"][cy, cx])
                    d = p - prev["p"][cy, cx]
                    d2 = _dot(d, d)
                    fin = np.isfinite(prev["M"][cy, cx]).all(-1) & np.isfinite(prev["Q"][cy, cx]).all(-1)
                    valid = cand & (ndot >= min_normal_dot) & (d2 <= tol2) & fin
                    b = (wx if dx else 1.0 - wx) * (wy if dy else 1.0 - wy)
                    near |= cand & ((np.abs(ndot - min_normal_dot) <= NEAR * abs(min_normal_dot)) | (np.abs(d2 - tol2) <= NEAR * tol2))
                    inherited |= valid & prev["taint"][cy, cx]
                    Wsum = Wsum + np.where(valid, b, 0.0)
                    Nh = Nh + np.where(valid, b * prev["N"][cy, cx], 0.0)
                    Mh = Mh + np.where(valid[..., None], b[..., None] * prev["M"][cy, cx], 0.0)
                    Qh = Qh + np.where(valid[..., None], b[..., None] * prev["Q"][cy, cx], 0.0)
            near |= ok & (np.abs(Wsum - MIN_WEIGHT) <= NEAR * MIN_WEIGHT)
        finite = np.isfinite(c).all(-1)
        history = finite & (Wsum >= MIN_WEIGHT)
        Wd = np.where(history, Wsum, 1.0)
        mh, qh, nh = Mh / Wd[..., None], Qh / Wd[..., None], Nh / Wd
        if clamp is not None:                                        # clause 3a
            lo, hi, _ = neighbourhood_box(c, in_tiles, clamp["radius"], clamp["gamma"], clamp["floor"])
            mc = np.where(mh < lo, lo, np.where(mh > hi, hi, mh))
            clamped = history & (mc != mh).any(-1)
            scale = np.maximum(np.abs(lo), np.abs(hi))
            near |= history & ((np.abs(mh - lo) <= NEAR * scale) | (np.abs(mh - hi) <= NEAR * scale)).any(-1)
            vh = qh - mh * mh
            qc = mc * mc + np.where(vh > 0.0, vh, 0.0)
            mh, qh = np.where(clamped[..., None], mc, mh), np.where(clamped[..., None], qc, qh)
            nh = np.where(clamped, np.minimum(nh, float(clamp["clamped_history"])), nh)
        N = np.where(history, np.minimum(nh + 1.0, float(max_history)), np.where(finite, 1.0, 0.0))
        Nd = np.where(history, N, 1.0)[..., None]
        cc = c * c
        M = np.where(history[..., None], mh + (c - mh) / Nd, c)
        Q = np.where(history[..., None], qh + (cc - qh) / Nd, cc)
    t3, h3 = in_tiles[..., None], (in_tiles & hit)[..., None]
    return dict(M=np.where(t3, M, 0.0), Q=np.where(t3, Q, 0.0), N=np.where(in_tiles, N, 0.0), p=np.where(h3, p, 0.0), n=np.where(h3, n, 0.0),
                leaf=np.where(in_tiles, leaf, -1).astype(np.int32), plane=plane, taint=(near | inherited) & in_tiles, history=history & in_tiles,
                clamped=clamped & in_tiles)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_the_clamp():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"typedef struct ft_temporal_clamp_params\s*\{\s*int32_t radius, clamped_history;\s*double gamma, floor;\s*\}\s*ft_temporal_clamp_params;", hdr)
    assert re.search(r"int32_t ft_temporal_set_clamp\(ft_context\* ctx, const ft_temporal_clamp_params\* params\);", hdr)
    assert re.search(r"int32_t ft_temporal_clamp_status\(ft_context\* ctx, int64_t out\[2\]\);", hdr)
    assert "#define FT_ABI_VERSION 2" in hdr
    lib = C.CDLL(ft.HIP_LIB)
    for name in ("ft_temporal_set_clamp", "ft_temporal_clamp_status"):
        assert hasattr(lib, name), name
    assert C.sizeof(_capi.ft_temporal_clamp_params) == 24
    assert _capi.TEMPORAL_CLAMP_DEFAULTS == dict(radius=1, clamped_history=1, gamma=1.0, floor=1e-4)
    assert _capi.TEMPORAL_DEFAULTS == dict(max_history=32, to_frame=0, min_normal_dot=0.9, position_tolerance_px=4.0) and C.sizeof(_capi.ft_temporal_params) == 24
    for name in ("temporal_set_clamp", "temporal_clamp_status"):
        assert callable(getattr(ft.Context, name)), name


def test_arguments_are_checked_in_order_before_the_device():
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    ctx.commit()
    lib = ft.hip_lib()
    inf, nan = float("inf"), float("nan")

    def call(null_ctx=False, **kw):
        p = _capi.ft_temporal_clamp_params()
        for k, v in {**_capi.TEMPORAL_CLAMP_DEFAULTS, **kw}.items():
            setattr(p, k, v)
        return lib.ft_temporal_set_clamp(None if null_ctx else ctx._ctx, C.byref(p))

    bad = [dict(radius=0), dict(radius=4), dict(radius=-1), dict(clamped_history=-1), dict(gamma=nan), dict(gamma=inf), dict(gamma=-0.5),
           dict(floor=nan), dict(floor=inf), dict(floor=-1e-9)]
    assert call(null_ctx=True) == -1 and call(null_ctx=True, radius=9) == -1 and lib.ft_temporal_set_clamp(None, None) == -1
    for kw in bad:                                                   # each alone: invalid, before the missing device (-2) and the missing begin (-5)
        assert call(**kw) == -1, kw
    for a in bad:                                                    # ... and combined with a later one
        for b in bad:
            assert call(**{**b, **a}) == -1, (a, b)
    assert call() == -2 and call(radius=3, clamped_history=0, gamma=0.0, floor=0.0) == -2 and call(radius=2, gamma=7.0) == -2
    assert lib.ft_temporal_set_clamp(ctx._ctx, None) == -2           # params == NULL is valid: off
    out = (C.c_int64 * 2)()
    assert lib.ft_temporal_clamp_status(None, out) == -1 and lib.ft_temporal_clamp_status(ctx._ctx, None) == -1
    assert lib.ft_temporal_clamp_status(ctx._ctx, out) == -2
    with pytest.raises(ft.FtError) as e:
        ctx.temporal_set_clamp(radius=2)
    assert e.value.status == -2
    with pytest.raises(ft.FtError) as e:
        ctx.temporal_set_clamp(None)
    assert e.value.status == -2
    with pytest.raises(ValueError):
        ctx.temporal_set_clamp(history=3)
    with pytest.raises(ValueError):
        ctx.temporal_set_clamp(off=True, radius=2)
    ctx.close()


def _random_state(rng, h, w, plane):
    st = new_state(h, w)
    st["M"], st["N"] = rng.uniform(0.0, 1.0, (h, w, 3)), rng.integers(0, 6, (h, w)).astype(np.float64)
    st["Q"] = st["M"] * st["M"] + rng.uniform(-0.01, 0.05, (h, w, 3))
    st["leaf"] = rng.integers(-1, 3, (h, w)).astype(np.int32)
    st["plane"] = plane
    return st


def test_with_the_clamp_off_the_restatement_is_test_temporals():
    rng = np.random.default_rng(41)
    h, w = 9, 13
    cam = ft.make_camera((1, 2, -7), (0.5, 0, 3), (0, 1, 0), H.deg(50), 1.3)
    pl = image_plane(cam, w, h)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    for trial in range(20):
        prev = _random_state(rng, h, w, pl if trial else None)
        p, n, _ = _flat_inputs(pl, xs + rng.uniform(-1.5, 1.5, (h, w)), ys + rng.uniform(-1.5, 1.5, (h, w)))
        prev["p"], prev["n"] = p + rng.normal(size=p.shape) * 0.02, n
        leaf = rng.integers(-1, 3, (h, w)).astype(np.int32)
        c = rng.uniform(0.0, 1.0, (h, w, 3))
        c[rng.integers(0, h), rng.integers(0, w), rng.integers(0, 3)] = np.nan
        tiles = rng.uniform(size=(h, w)) < 0.8
        kw = dict(max_history=int(rng.integers(1, 8)), min_normal_dot=0.9, position_tolerance_px=float(rng.uniform(0.5, 6.0)))
        want, got = reference(prev, pl, c, p, n, leaf, tiles, **kw), reference_clamped(prev, pl, c, p, n, leaf, tiles, None, **kw)
        for key in ("M", "Q", "N", "p", "n", "leaf", "taint", "history"):
            assert np.array_equal(np.ascontiguousarray(want[key]).view(np.uint8), np.ascontiguousarray(got[key]).view(np.uint8)), (trial, key)
        assert not got["clamped"].any() and (trial == 0 or got["history"].any())


def _still(pl, h, w, M, N=None, Q=None):
    """A flat patch seen twice from the same camera: the state after a call that stored M (N, Q), and the inputs of the next call."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    p, n, leaf = _flat_inputs(pl, xs, ys)
    st = new_state(h, w)
    st.update(M=M.copy(), Q=(M * M if Q is None else Q).copy(), N=np.full((h, w), 1.0) if N is None else N.copy(), p=p, n=n, leaf=leaf, plane=pl)
    return st, p, n, leaf


def test_restatement_on_hand_worked_cases():
    h, w = 5, 6
    cam = ft.make_camera((1, 2, -7), (0.5, 0, 3), (0, 1, 0), H.deg(50), 1.3)
    pl = image_plane(cam, w, h)
    on = np.ones((h, w), dtype=bool)
    tight = dict(rtol=1e-12, atol=0)
    flat = np.full((h, w, 3), 0.5)
    # a flat neighbourhood: sd = 0 and the box is mu +- floor.  A history half a floor away is not clamped, one three floors away is:
    # it is moved to hi = 0.5 + 1e-4, keeps clamped_history = 1 of its 5 calls, and the blend halves what is left
    for off, hit in ((0.5e-4, False), (3e-4, True)):
        st, p, n, leaf = _still(pl, h, w, flat + off, N=np.full((h, w), 5.0))
        got = reference_clamped(st, pl, flat, p, n, leaf, on, dict(AGGRESSIVE))
        assert got["history"].all() and got["clamped"].all() == hit and got["clamped"].any() == hit and not got["taint"].any()
        if hit:
            assert np.allclose(got["N"], 2.0, **tight) and np.allclose(got["M"], 0.5 + 0.5e-4, **tight)
        else:
            plain = reference(st, pl, flat, p, n, leaf, on)
            assert np.allclose(got["N"], 6.0, **tight) and all(np.array_equal(got[k], plain[k]) for k in ("M", "Q", "N"))
    lo, hi, k = neighbourhood_box(flat, on, 1, 1.0, 1e-4)
    assert np.array_equal(lo, flat - 1e-4) and np.array_equal(hi, flat + 1e-4)
    assert k[0, 0] == 4 and k[0, 2] == 6 and k[2, 2] == 9
    # one bright tap among eight equal ones: mu = 1/9, sd = sqrt(8)/9, and the bright pixel sits sqrt(8) = sqrt(k - 1) standard deviations
    # from the mean - Samuelson's bound, met.  A history that equals the frame is clamped just below gamma = sqrt(8), not just above
    spike = np.zeros((h, w, 3))
    spike[2, 3] = 1.0
    lo, hi, k = neighbourhood_box(spike, on, 1, 1.0, 0.0)
    assert k[2, 3] == 9 and np.allclose(hi[2, 3] - lo[2, 3], 2.0 * math.sqrt(8.0) / 9.0, **tight) and np.allclose(lo[2, 3] + hi[2, 3], 2.0 / 9.0, **tight)
    st, p, n, leaf = _still(pl, h, w, spike)
    for gamma, hit in ((math.sqrt(8.0) * (1.0 + 1e-6), False), (math.sqrt(8.0) * (1.0 - 1e-6), True)):
        got = reference_clamped(st, pl, spike, p, n, leaf, on, dict(radius=1, clamped_history=1, gamma=gamma, floor=0.0))
        want = np.zeros((h, w), dtype=bool)
        want[2, 3] = hit
        assert np.array_equal(got["clamped"], want), gamma
    assert not reference_clamped(st, pl, spike, p, n, leaf, on, dict(radius=2, clamped_history=1, gamma=math.sqrt(24.0) * (1.0 + 1e-6), floor=0.0))["clamped"].any()
    # a NaN tap is left out of its neighbours' boxes: they are those of the other 8 (or fewer) taps; the NaN pixel itself stores N = 0
    rng = np.random.default_rng(8)
    c = rng.uniform(0.1, 1.0, (h, w, 3))
    bad = c.copy()
    bad[2, 2, 1] = np.nan
    lo, hi, k = neighbourhood_box(bad, on, 1, 1.0, 1e-4)
    assert k[2, 2] == 8 and k[1, 1] == 8 and k[2, 3] == 8 and k[0, 0] == 4 and k[4, 5] == 4 and k[2, 4] == 9
    taps = [c[y, x] for y in (0, 1, 2) for x in (0, 1, 2) if (y, x) != (2, 2)]   # the neighbourhood of (1, 1) without (2, 2), in the summation order
    mu = sum(taps[1:], taps[0]) / 8.0
    sd = np.sqrt(sum([t * t for t in taps[1:]], taps[0] * taps[0]) / 8.0 - mu * mu)
    assert np.array_equal(lo[1, 1], mu - (1.0 * sd + 1e-4)) and np.array_equal(hi[1, 1], mu + (1.0 * sd + 1e-4))
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    st, p, n, leaf = _still(pl, h, w, c)
    got = reference_clamped(st, pl, bad, p, n, leaf, on, dict(AGGRESSIVE))
    assert got["N"][2, 2] == 0.0 and np.isnan(got["M"][2, 2, 1]) and not got["clamped"][2, 2] and np.isfinite(np.delete(got["M"].reshape(-1, 3), 2 * w + 2, axis=0)).all()
    # a tap outside T is left out as well: with columns 4 and 5 outside, column 3 sees six taps and the corner (0, 3) four
    tiles = on.copy()
    tiles[:, 4:] = False
    lo_t, hi_t, k_t = neighbourhood_box(c, tiles, 1, 1.0, 1e-4)
    assert k_t[2, 3] == 6 and k_t[0, 3] == 4 and k_t[2, 2] == 9
    narrow = neighbourhood_box(c[:, :4], on[:, :4], 1, 1.0, 1e-4)   # ... exactly as if the frame ended there
    assert np.array_equal(lo_t[:, :4], narrow[0]) and np.array_equal(hi_t[:, :4], narrow[1])
    got = reference_clamped(st, pl, c, p, n, leaf, tiles, dict(AGGRESSIVE))
    assert (got["N"][:, 4:] == 0.0).all() and not got["clamped"][:, 4:].any()
    # a corner pixel with r = 3 sees 4 x 4 = 16 taps of the 5 x 6 frame, the pixel (2, 3) 5 x 6 = 30 (rows 0 .. 4, columns 0 .. 5)
    lo3, hi3, k3 = neighbourhood_box(c, on, 3, 1.0, 0.0)
    assert k3[0, 0] == 16 and k3[4, 5] == 16 and k3[2, 3] == 30 and k3[2, 2] == 30 and k3[0, 5] == 16
    corner = c[:4, :4].reshape(-1, 3)
    mu = sum(list(corner[1:]), corner[0]) / 16.0
    assert np.array_equal(lo3[0, 0] + hi3[0, 0], (mu - np.sqrt(np.maximum(sum([t * t for t in corner[1:]], corner[0] * corner[0]) / 16.0 - mu * mu, 0.0)))
                          + (mu + np.sqrt(np.maximum(sum([t * t for t in corner[1:]], corner[0] * corner[0]) / 16.0 - mu * mu, 0.0))))
    # clamped_history: 1 keeps one call of the history (N = 2, half-way between the moved mean and c), 0 restarts the pixel at M = c
    dark = np.full((h, w, 3), 0.1)
    st, p, n, leaf = _still(pl, h, w, dark, N=np.full((h, w), 7.0))
    one = reference_clamped(st, pl, flat, p, n, leaf, on, dict(AGGRESSIVE, clamped_history=1))
    zero = reference_clamped(st, pl, flat, p, n, leaf, on, dict(AGGRESSIVE, clamped_history=0))
    assert one["clamped"].all() and zero["clamped"].all()
    assert np.allclose(one["N"], 2.0, **tight) and np.allclose(one["M"], 0.5 - 0.5e-4, **tight)
    assert (zero["N"] == 1.0).all() and np.array_equal(zero["M"], flat) and zero["history"].all()
    assert np.allclose(reference(st, pl, flat, p, n, leaf, on)["M"], 0.1 + 0.4 / 8.0, **tight)    # without the clamp the old colour lingers
    # Q_c: the variance of the history rides along around the moved mean (Vh = 0.03), and a negative Vh counts as none
    for vh in (0.03, -0.02):
        st, p, n, leaf = _still(pl, h, w, dark, N=np.full((h, w), 7.0), Q=dark * dark + vh)
        got = reference_clamped(st, pl, flat, p, n, leaf, on, dict(AGGRESSIVE))
        mc = 0.5 - 1e-4
        qc = mc * mc + max(vh, 0.0)
        assert got["clamped"].all() and np.allclose(got["Q"], qc + (0.25 - qc) / 2.0, **tight)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _step(ctx, st, pose_of_set, cam, w, h, spp, jit, sample, seed, inside, tiles=None, clamp=None, deformed=None, **accumulate):
    """render, the surfaces, accumulate, and the restatement's state after it (the taken-back point and normal where the scene moved or,
    with `deformed` - a function of the live and the history's matrices - where a mesh deformed)."""
    c, _ = ctx.render(cam, w, h, spp, jit, seed=seed)
    g = ctx.render_aov(cam, w, h, spp, jit, sample=sample, seed=seed, tiles=tiles, channels=["p", "n", "leaf", "triangle"])
    out, stats = ctx.temporal_accumulate(cam, spp, jit, sample=sample, seed=seed, out=np.full((h, w, 3), 7.0), **accumulate)
    now = _matrices(ctx)
    then = pose_of_set or now
    D, A, moved = motion(now[0], now[1], *then)
    pr, nr = taken_back(g["p"], g["n"], g["leaf"], D, A, moved)
    thin = np.zeros(inside.shape, dtype=bool)
    if deformed is not None:
        d = deformed(now, then)
        pd, nd, followed = taken_back_deformed(g["p"], g["n"], g["leaf"], g["triangle"], **d)
        pr, nr = np.where(followed[..., None], pd, pr), np.where(followed[..., None], nd, nr)
        thin = sliver_pixels(g["leaf"], g["triangle"], **d)
    st = reference_clamped(st, image_plane(cam, w, h), c, pr, nr, g["leaf"], inside, clamp)
    h3 = (inside & (g["leaf"] >= 0))[..., None]
    st["p"], st["n"] = np.where(h3, g["p"], 0.0), np.where(h3, g["n"], 0.0)   # clause 6 stores the current surface
    st["taint"] = st["taint"] | (thin & inside)
    return st, now, dict(c=c, g=g, out=out, stats=stats)


def _clamped_count_agrees(ctx, st, radius):
    status = ctx.temporal_clamp_status()
    left_out = int(st["taint"].sum())
    want = int((st["clamped"] & ~st["taint"]).sum())
    assert status["radius"] == radius and want <= status["clamped"] <= want + left_out, (status, want, left_out)
    return status["clamped"]


def _sequence(hip, cams, w, h, spp, tiles, clamp, what):
    """Parity of the device with the restatement along `cams` in the scene the context holds; returns the clamped counts and the pixels with
    history per call."""
    jit, sample = ft.jitter_pattern(spp), spp - 1
    inside = _mask(tiles, w, h)
    hip.temporal_begin(w, h, tiles=tiles)
    assert hip.temporal_clamp_status() == {"radius": 0, "clamped": 0}
    hip.temporal_set_clamp(**clamp)
    st, pose = new_state(h, w), None
    worst, share, counts, with_history = 0.0, 0.0, [], []
    for k, cam in enumerate(cams):
        st, pose, io = _step(hip, st, pose, cam, w, h, spp, jit, sample, 100 + k, inside, tiles=tiles, clamp=clamp)
        left_out = int(st["taint"].sum())
        share = max(share, left_out / int(inside.sum()))
        err, M, _, _ = _compare(hip, st, inside & ~st["taint"], f"{what} call {k}")
        worst = max(worst, err)
        assert np.array_equal(io["out"][inside], M[inside], equal_nan=True) and (io["out"][~inside] == 7.0).all()
        status = hip.temporal_status()
        assert status["calls"] == k + 1 and status["pixels"] == int(inside.sum()) and abs(status["with_history"] - int(st["history"].sum())) <= left_out
        counts.append(_clamped_count_agrees(hip, st, clamp["radius"]))
        with_history.append(status["with_history"])
        n_rects = 1 if tiles is None else len(tiles)
        assert io["stats"]["n_launches"] >= 2 + n_rects and 0.0 < io["stats"]["trace_kernel_ms"] < io["stats"]["kernel_ms"]
    print(f"temporal clamp parity {what}: worst error {worst:.3e} x the bound, left out {share:.5%} of the tile pixels, pixels with history per call {with_history}, "
          f"of them clamped {counts}")
    assert share <= LEFT_OUT_CAP, f"{share:.5%} of the tile pixels lie within {NEAR} of a threshold"
    assert counts[0] == 0
    hip.temporal_end()
    return counts, with_history


# ---------------------------------------------------------------------------------------------------------------- 1. device against restatement
@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("tiles", [None, CLIPPED], ids=["frame", "tiles"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("name", ["bunny", "sample-soft"])
def test_device_matches_the_numpy_restatement(hip, name, spp, tiles, radius):
    counts, with_history = _sequence(hip, orbit(_load(hip, name).camera, 6), W, Hh, spp, tiles, dict(AGGRESSIVE, radius=radius),
                                     f"{name} x{spp} {'tiles' if tiles else 'frame'} r{radius}")
    assert tiles is not None or (min(with_history[1:]) > 0 and max(counts) > 0)    # the orbit does reproject, and gamma 1 does clamp


@pytest.mark.gpu
def test_device_matches_the_restatement_over_several_windows(hip):
    """chunk_samples 4096: the 14 400 pixels are cut into four windows; the boxes are taken once, before the first."""
    cams = orbit(_load(hip, "sample-soft").camera, 4)
    hip.set_option("chunk_samples", 4096)
    try:
        counts, _ = _sequence(hip, cams, W, Hh, 1, None, dict(AGGRESSIVE, radius=2), "sample-soft, four windows")
    finally:
        hip.set_option("chunk_samples", 16 << 20)
    assert max(counts) > 0


@pytest.mark.gpu
def test_device_matches_the_restatement_where_the_halo_outgrows_the_frame(hip):
    cams = orbit(_load(hip, "sample-soft", pinhole=True).camera, 4, step_deg=0.5)
    _sequence(hip, cams, 5, 3, 1, None, dict(AGGRESSIVE, radius=3), "sample-soft 5 x 3, r3")


@pytest.mark.gpu
def test_device_matches_the_restatement_on_tiles_that_show_surfaces(hip):
    """The tiles of bunny and sample-soft show little but sky; test_temporal_motion.py's scene puts its mesh and its cube into
    them, so here the in-T test of the boxes decides about histories that exist."""
    _build(hip, _pose(0.0))
    counts, with_history = _sequence(hip, orbit(_motion_camera(), 4), W, Hh, 1, CLIPPED, dict(AGGRESSIVE, radius=2), "motion scene, tiles, r2")
    assert min(with_history[1:]) > 0


# ---------------------------------------------------------------------------------------------------------------- 2. borders
@pytest.mark.gpu
def test_a_non_finite_pixel_is_left_out_of_its_neighbours_boxes(hip, golden):
    """The NaN scene of test_temporal.py's test_non_finite_pixels_stay_where_they_are, with the clamp on."""
    case = [c for c in golden["hand_derived_shading"]["cases"] if c["name"] == "specular_negative_base_fractional_exponent_is_nan"][0]
    H.build_described_scene(hip, case["objects"], case["lights"])
    cams = orbit(ft.make_camera((0, 0, -3), (0, 0, 0), (0, 1, 0), H.deg(40.0), 1.0), 3)
    jit = np.zeros((1, 2))
    everywhere = _mask(None, 64, 64)
    for radius in (1, 3):
        clamp = dict(AGGRESSIVE, radius=radius)
        hip.temporal_begin(64, 64)
        hip.temporal_set_clamp(**clamp)
        st, pose = new_state(64, 64), None
        for k, cam in enumerate(cams):
            st, pose, io = _step(hip, st, pose, cam, 64, 64, 1, jit, 0, ft.DEFAULT_SEED, everywhere, clamp=clamp)
            bad = np.isnan(io["c"]).any(-1)
            assert bad.any() and not bad.all()
            lo, hi, count = neighbourhood_box(io["c"], everywhere, radius, clamp["gamma"], clamp["floor"])
            beside = _grown(bad, radius) & ~bad
            assert np.isfinite(lo[beside]).all() and np.isfinite(hi[beside]).all() and (count[beside] < (2 * radius + 1) ** 2).all()
            assert int(st["taint"].sum()) <= LEFT_OUT_CAP * 64 * 64
            _, M, _, N = _compare(hip, st, everywhere & ~st["taint"], f"NaN frame r{radius} call {k}")
            assert np.array_equal(~np.isfinite(M).all(-1), bad) and (N[bad] == 0.0).all() and (N[~bad] >= 1.0).all()
            assert np.array_equal(np.isnan(io["out"]), np.isnan(M))
            _clamped_count_agrees(hip, st, radius)
        assert hip.temporal_status()["with_history"] > 0
        hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 3. the ghost goes
GHOST_CAM = dict(o=(0.0, 4.0, -9.0), look_at=(0.0, 0.0, 0.0))
GHOST_SPHERE = [(-1.5, 1.5, 0.0), (2.5, 1.5, 0.0)]                   # before and after the move: the shadow leaves its place


def _ghost_camera():
    return ft.make_camera(GHOST_CAM["o"], GHOST_CAM["look_at"], (0.0, 1.0, 0.0), H.deg(50.0), 16.0 / 9.0)


def _ghost_scene(ctx):
    """A ground plane, a unit sphere under a translate above it, one directional light."""
    ctx.clear()
    ground = ctx.material(ctx.primitive(ft.PLANE), colour=(0.6, 0.6, 0.55))
    node = ctx.transform([("translate", GHOST_SPHERE[0])], ctx.primitive(ft.SPHERE))
    ctx.set_objects(ctx.group([ground, ctx.material(node, colour=(0.9, 0.3, 0.2))]))
    ctx.add_directional((0.3, -1.0, 0.4), (1.0, 1.0, 1.0))
    ctx.commit()
    return node


def _luminance(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _range3x3(c):
    """Per pixel and channel max - min of c over the pixel's 3 x 3 taps that lie in the frame."""
    h, w = c.shape[:2]
    hi, lo = np.full((h + 2, w + 2, 3), -np.inf), np.full((h + 2, w + 2, 3), np.inf)
    hi[1:-1, 1:-1], lo[1:-1, 1:-1] = c, c
    return (np.max([hi[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
            - np.min([lo[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0))


def _ghost_run(hip, clamp, move=True, calls=5):
    """Four calls, the sphere moves, one more (or `calls` without a move).  Per call: frame, surfaces, fetch, the restatement's state."""
    node = _ghost_scene(hip)
    cam, jit = _ghost_camera(), np.zeros((1, 2))
    everywhere = _mask(None)
    hip.temporal_begin(W, Hh)
    if clamp is not None:
        hip.temporal_set_clamp(**clamp)
    st, pose, out = new_state(Hh, W), None, []
    for k in range(calls):
        if move and k == calls - 1:
            hip.set_transform(node, [("translate", GHOST_SPHERE[1])])
            hip.commit_moved()
        st, pose, io = _step(hip, st, pose, cam, W, Hh, 1, jit, 0, 7, everywhere, clamp=clamp)
        M, se, N = hip.temporal_fetch()
        out.append(dict(io, M=M, se=se, N=N, st=st, status=hip.temporal_status(), clamp=hip.temporal_clamp_status()))
    hip.temporal_end()
    return out


@pytest.mark.gpu
def test_the_ghost_of_a_moved_shadow_goes(hip):
    """A sphere slides over a lit plane under a still camera; frames are free of noise (1 spp, jitter 0).  Where its shadow lay, the plane's
    history is valid and dark.  Without the clamp the old shadow lingers at 4/5 of its depth; with it every such pixel is within
    1.5 x (the range of the current frame over its 3 x 3 taps) + floor of the current frame: M_c lies in [lo, hi], sd <= range / 2, mu and
    c lie in [min, max], and |M - c| = |M_c - c| (1 - 1/N)."""
    on, off = _ghost_run(hip, dict(AGGRESSIVE)), _ghost_run(hip, None)
    last, before = on[-1], on[-2]
    assert all(np.array_equal(a["c"], b["c"], equal_nan=True) and np.array_equal(a["g"]["leaf"], b["g"]["leaf"]) for a, b in zip(on, off))
    plane_leaf = int(last["g"]["leaf"][Hh - 1, W // 2])
    plane = (last["g"]["leaf"] == plane_leaf) & (before["g"]["leaf"] == plane_leaf)
    assert plane_leaf >= 0 and plane.sum() > W * Hh // 4
    c = last["c"]
    P = plane & last["st"]["history"] & (_luminance(c) > 2.0 * _luminance(before["c"]))
    assert P.sum() > 0, "no plane pixel left the shadow"
    bound = 1.5 * _range3x3(c) + AGGRESSIVE["floor"] + 1e-12
    err_on, err_off = np.abs(last["M"] - c), np.abs(off[-1]["M"] - c)
    print(f"temporal clamp ghost: {int(P.sum())} plane pixels left the shadow; |M - c| there at most {float(err_on[P].max()):.3e} with the clamp "
          f"(bound at that pixel {float(bound[P][np.argmax(err_on[P].max(-1))].max()):.3e}), {float(err_off[P].max()):.3e} without; "
          f"N there {float(last['N'][P].min())} .. {float(last['N'][P].max())} with, {float(off[-1]['N'][P].min())} .. {float(off[-1]['N'][P].max())} without; "
          f"{last['clamp']['clamped']} pixels clamped in the last call")
    assert (err_on[P] <= bound[P]).all()
    assert (last["N"][P] <= 2.0).all()
    assert (err_off[P] > bound[P]).any(), "the scene shows no ghost without the clamp either"
    assert off[-1]["clamp"] == {"radius": 0, "clamped": 0} and last["clamp"]["radius"] == 1 and last["clamp"]["clamped"] >= int((P & ~last["st"]["taint"]).sum())
    # elsewhere: a plane pixel that was lit before and after and that the clamp never reached - neither itself nor, a ring further per
    # call, through a tap (with a still camera the taps lie in the pixel's 3 x 3 neighbourhood) - has the bits of the unclamped run
    reached = np.zeros((Hh, W), dtype=bool)
    for call in on:
        reached = _grown(reached, 1) | _grown(call["st"]["clamped"] | call["st"]["taint"], 1)
    lit = plane & ~reached & (_luminance(c) <= 2.0 * _luminance(before["c"])) & (_luminance(before["c"]) <= 2.0 * _luminance(c)) & (_luminance(c) > 0.0)
    assert lit.sum() > W * Hh // 8
    for name in ("M", "se", "N"):
        assert np.array_equal(last[name][lit], off[-1][name][lit]), name
    # ft_temporal_status: the clamp changes no history's validity, and can only shorten
    for a, b in zip(on, off):
        assert all(a["status"][key] == b["status"][key] for key in ("calls", "pixels", "with_history")) and a["status"]["at_max_history"] <= b["status"]["at_max_history"]


# ---------------------------------------------------------------------------------------------------------------- 4. a held view loses nothing
@pytest.mark.gpu
def test_a_held_view_loses_nothing(hip):
    """gamma 3 >= sqrt(8): by Samuelson's inequality no history that equals the frame can be clamped at r = 1."""
    wide = dict(radius=1, clamped_history=1, gamma=3.0, floor=1e-6)
    on, off = _ghost_run(hip, wide, move=False, calls=6), _ghost_run(hip, None, move=False, calls=6)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a["clamp"] == {"radius": 1, "clamped": 0}, k
        assert not a["st"]["clamped"].any()
        assert all(np.array_equal(a[name], b[name], equal_nan=True) for name in ("M", "se", "N", "out")), k
        assert a["status"] == b["status"]
    assert on[-1]["status"]["with_history"] > W * Hh // 2 and float(on[-1]["N"].max()) > 5.5


# ---------------------------------------------------------------------------------------------------------------- 5. off is off
@pytest.mark.gpu
def test_switched_off_the_next_call_is_the_unclamped_restatement(hip):
    scene = _load(hip, "sample-soft", pinhole=True)
    cams, jit = orbit(scene.camera, 4), np.zeros((1, 2))
    everywhere = _mask(None)
    hip.temporal_begin(W, Hh)
    hip.temporal_set_clamp(radius=2)
    for k, cam in enumerate(cams[:3]):
        hip.render(cam, W, Hh, 1, jit, seed=50 + k, fetch=False)
        hip.temporal_accumulate(cam, 1, jit, seed=50 + k, fetch=False)
    assert hip.temporal_clamp_status()["radius"] == 2 and hip.temporal_clamp_status()["clamped"] > 0
    # the state the device holds, from what it reports: M, N, Q = se^2 N + M^2 (M^2 where N < 2), and the surfaces of the last call
    M, se, N = hip.temporal_fetch()
    p, n, leaf = _surfaces(hip, cams[2], W, Hh, 1, jit, 0, 52)
    st = new_state(Hh, W)
    st.update(M=M, Q=np.where((N >= 2.0)[..., None], se * se * N[..., None] + M * M, M * M), N=N, p=p, n=n, leaf=leaf, plane=image_plane(cams[2], W, Hh))
    hip.temporal_set_clamp(None)
    assert hip.temporal_clamp_status() == {"radius": 0, "clamped": hip.temporal_clamp_status()["clamped"]}
    c, _ = hip.render(cams[3], W, Hh, 1, jit, seed=53)
    p, n, leaf = _surfaces(hip, cams[3], W, Hh, 1, jit, 0, 53)
    hip.temporal_accumulate(cams[3], 1, jit, seed=53, fetch=False)
    want = reference(st, image_plane(cams[3], W, Hh), c, p, n, leaf, everywhere)
    assert int(want["taint"].sum()) <= LEFT_OUT_CAP * W * Hh
    _compare(hip, want, everywhere & ~want["taint"], "the call after the clamp was switched off")
    assert hip.temporal_clamp_status() == {"radius": 0, "clamped": 0} and hip.temporal_status()["with_history"] > 0
    # a second begin starts with the clamp off, and whatever ends the accumulation drops it
    hip.temporal_set_clamp(radius=3)
    hip.temporal_begin(W, Hh)
    assert hip.temporal_clamp_status() == {"radius": 0, "clamped": 0}
    hip.temporal_end()
    for call in (hip.temporal_clamp_status, hip.temporal_set_clamp, lambda: hip.temporal_set_clamp(None)):
        with pytest.raises(ft.FtError) as e:
            call()
        assert e.value.status == -5
    two = ft.Context(device=[0, 0])
    try:
        scene.lower(two)
        with pytest.raises(ft.FtError) as e:
            two.temporal_set_clamp()
        assert e.value.status == -4
        with pytest.raises(ft.FtError) as e:
            two.temporal_set_clamp(radius=0)
        assert e.value.status == -1
    finally:
        two.close()


# ---------------------------------------------------------------------------------------------------------------- 6. composition
@pytest.mark.gpu
def test_the_clamp_composes_with_followed_triangles(hip):
    """test_temporal_deform.py's scene and deformation under "temporal_follow_deformed" = 1, the clamp on: the restatement is fed the point
    and the normal taken back through the snapshot."""
    rec = Recorder(hip)
    _build(rec, _pose(0.0))
    mesh = rec.meshes[0]
    cam, jit = _motion_camera(), np.zeros((1, 2))
    everywhere = _mask(None)
    clamp = dict(AGGRESSIVE, radius=2)
    try:
        hip.set_option(FOLLOW_OPTION, 1)
        mesh_leaf, n_leaves = _mesh_leaf(hip, cam), hip.scene_info()["leaves"]
        hip.temporal_begin(W, Hh)
        hip.temporal_set_clamp(**clamp)
        st, pose, share, followed_px = new_state(Hh, W), None, 0.0, 0
        for k in range(4):
            deformed = None
            if k > 0:
                hip.set_mesh_triangles(mesh, _shape(float(k)))
                hip.commit_deformed()
                deformed = lambda now, then, k=k: _deformed(n_leaves, mesh_leaf, _shape(float(k)), _shape(float(k - 1)), now, then)
            st, pose, io = _step(hip, st, pose, cam, W, Hh, 1, jit, 0, 100 + k, everywhere, clamp=clamp, deformed=deformed)
            share = max(share, int(st["taint"].sum()) / (W * Hh))
            _compare(hip, st, everywhere & ~st["taint"], f"clamp on followed triangles, call {k}")
            _clamped_count_agrees(hip, st, 2)
            if k > 0:
                followed_px += int((st["history"] & (io["g"]["leaf"] == mesh_leaf)).sum())
        print(f"temporal clamp on followed triangles: left out {share:.5%}, pixels with history on the deformed mesh {followed_px}")
        assert share <= LEFT_OUT_CAP and followed_px > 0
        hip.temporal_end()
    finally:
        hip.set_option(FOLLOW_OPTION, 0)


# ---------------------------------------------------------------------------------------------------------------- 7. output forms
@pytest.mark.gpu
def test_output_forms_with_the_clamp_on(hip):
    scene = _load(hip, "moon")
    cams, jit = orbit(scene.camera, 3, step_deg=0.2), ft.jitter_pattern(2)
    inside = _mask(CLIPPED)
    for to_frame in (0, 1):
        hip.temporal_begin(W, Hh, tiles=CLIPPED)
        hip.temporal_set_clamp(**AGGRESSIVE)
        twin = ft.Context(device=0)                                  # the same sequence, asked for bytes
        try:
            scene.lower(twin)
            twin.temporal_begin(W, Hh, tiles=CLIPPED)
            twin.temporal_set_clamp(**AGGRESSIVE)
            clamped = 0
            for k, cam in enumerate(cams):
                c, _ = hip.render(cam, W, Hh, 2, jit, seed=k)
                twin.render(cam, W, Hh, 2, jit, seed=k, fetch=False)
                f64, _ = hip.temporal_accumulate(cam, 2, jit, seed=k, to_frame=to_frame, out=np.full((Hh, W, 3), 7.0))
                u8, _ = twin.temporal_accumulate(cam, 2, jit, seed=k, rgba8=True, out=np.full((Hh, W, 4), 9, dtype=np.uint8))
                assert np.array_equal(u8[inside], ft.quantise_rgba8(f64)[inside]) and (u8[~inside] == 9).all() and (f64[~inside] == 7.0).all()
                assert hip.temporal_clamp_status() == twin.temporal_clamp_status()
                clamped += hip.temporal_clamp_status()["clamped"]
                frame = hip.fetch_frame(np.zeros((Hh, W, 3)))
                if to_frame:
                    assert np.array_equal(frame[inside], f64[inside]) and np.array_equal(frame[~inside], c[~inside])
                else:
                    assert np.array_equal(frame, c)
                M, _, N = hip.temporal_fetch()
                assert np.array_equal(M[inside], f64[inside]) and (N[~inside] == 0.0).all() and (M[~inside] == 0.0).all()
                hip.render(cam, W, Hh, 2, jit, seed=k, fetch=False)
                _, stats = hip.temporal_accumulate(cam, 2, jit, seed=k, fetch=False)      # out == NULL
                assert stats["n_launches"] >= 2 + len(CLIPPED)
                twin.render(cam, W, Hh, 2, jit, seed=k, fetch=False)
                twin.temporal_accumulate(cam, 2, jit, seed=k, fetch=False)
            assert clamped > 0 and not np.array_equal(f64[inside], c[inside])
        finally:
            twin.close()
        hip.temporal_end()

"""ft_temporal_* (Context.temporal_*): the FP64 frames a host renders along a camera path accumulated on the device - each pixel's surface
point is projected into the previous call's image, the history found there is checked for being the same surface and blended with the new
frame.  `reference` below restates the definition of include/functracer_hip.h / DESIGN.md 12 in numpy; its inputs come from the public
API (render, render_aov), so it shares no code with k_temporal.

ft_temporal_fetch reports the mean of squares Q through the standard error only, so Q is compared as se^2 * max(N, 1) + M * M: that is Q
wherever the variance Q - M * M is not clamped at 0, and M * M (what a history of length 1 holds) where it is.

The GPU tests print the figures they assert on; what an MI355X gave is in DESIGN.md 12 "Measured"."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import helpers as H

W, Hh = 160, 90
TILES = [(8, 8, 16, 16), (101, 37, 13, 11), (150, 80, 20, 20)]       # those of test_denoise.py
MIN_WEIGHT = 1.0 / 16.0                                              # FT_TEMPORAL_MIN_WEIGHT
NEAR = 1e-9                                                          # a compared quantity this close (relative) to its threshold may fall either way
RTOL, ATOL = 1e-9, 1e-12
LEFT_OUT_CAP = 1e-3                                                  # share of tile pixels a case may leave out: a condition, not a measurement


# ---------------------------------------------------------------------------------------------------------------- the definition, in numpy
def image_plane(cam, res_h, res_v):
    """ImagePlane.create (Image.fs:48-81) of an ft_camera: o, i, j, k, the top-left pixel centre and the pixel size (sic: the width is
    divided by res_v - 1, the height by res_h - 1)."""
    def norm(v):
        l = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return v if l < 0.0000001 else (1.0 / l) * v
    o, look, up = np.array(cam.o[:]), np.array(cam.look_at[:]), np.array(cam.up[:])
    k = norm(look - o)
    i = norm(np.cross(up, k))
    j = np.cross(k, i)
    height = math.tan(cam.fov_y / 2.0) * 2.0
    width = height * cam.aspect_ratio
    ph, pw = height / (res_h - 1), width / (res_v - 1)
    return dict(o=o, i=i, j=j, k=k, pw=pw, ph=ph, tlx=-width / 2.0 + pw / 2.0, tly=height / 2.0 - ph / 2.0)


def ray_through_pixel(pl, x, y):
    """rayThroughPixel (Image.fs:83-89) at jitter 0; x, y may be fractional arrays.  Returns the (unnormalised) direction."""
    jx, jy = pl["tlx"] + np.asarray(x, dtype=np.float64) * pl["pw"], pl["tly"] - np.asarray(y, dtype=np.float64) * pl["ph"]
    return pl["k"] + jx[..., None] * pl["i"] + jy[..., None] * pl["j"]


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def project(pl, p):
    """Clause 1: (fx, fy, zc) of the points p[..., 3] in the image plane pl."""
    v = p - pl["o"]
    zc = _dot(v, pl["k"])
    with np.errstate(all="ignore"):
        fx = (_dot(v, pl["i"]) / zc - pl["tlx"]) / pl["pw"]
        fy = (pl["tly"] - _dot(v, pl["j"]) / zc) / pl["ph"]
    return fx, fy, zc


def new_state(h, w):
    """What ft_temporal_begin leaves: N = 0 everywhere, no previous image plane."""
    return dict(M=np.zeros((h, w, 3)), Q=np.zeros((h, w, 3)), N=np.zeros((h, w)), p=np.zeros((h, w, 3)), n=np.zeros((h, w, 3)),
                leaf=np.full((h, w), -1, dtype=np.int32), plane=None, taint=np.zeros((h, w), dtype=bool), history=np.zeros((h, w), dtype=bool))


def reference(prev, plane, c, p, n, leaf, in_tiles, max_history=32, min_normal_dot=0.9, position_tolerance_px=4.0):
    """One ft_temporal_accumulate: the state after it.  c, p, n: [h, w, 3]; leaf: [h, w] int; in_tiles: [h, w] bool.  Beside the set
    (M, Q, N, p, n, leaf) and the image plane the state carries `history` (tile pixels whose history was valid) and `taint`: tile pixels
    where one of the compared quantities of a tap (n.n', |dp|^2, W) lies within NEAR of its threshold, or that descend from such a pixel
    through a valid tap - the only pixels a correct implementation may disagree on."""
    h, w = leaf.shape
    hit = leaf >= 0
    Wsum, Nh = np.zeros((h, w)), np.zeros((h, w))
    Mh, Qh = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    near, inherited = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    with np.errstate(all="ignore"):
        if prev["plane"] is not None:
            pp = prev["plane"]
            fx, fy, zc = project(pp, p)
            ok = hit & (zc > 0.0) & (fx >= -1.0) & (fx < w) & (fy >= -1.0) & (fy < h)     # else none of the four taps is in the frame
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
        N = np.where(history, np.minimum(nh + 1.0, float(max_history)), np.where(finite, 1.0, 0.0))
        Nd = np.where(history, N, 1.0)[..., None]
        cc = c * c
        M = np.where(history[..., None], mh + (c - mh) / Nd, c)
        Q = np.where(history[..., None], qh + (cc - qh) / Nd, cc)
    t3, h3 = in_tiles[..., None], (in_tiles & hit)[..., None]
    return dict(M=np.where(t3, M, 0.0), Q=np.where(t3, Q, 0.0), N=np.where(in_tiles, N, 0.0), p=np.where(h3, p, 0.0), n=np.where(h3, n, 0.0),
                leaf=np.where(in_tiles, leaf, -1).astype(np.int32), plane=plane, taint=(near | inherited) & in_tiles, history=history & in_tiles)


def stderr_of(M, Q, N):
    """ft_temporal_fetch's standard error: sqrt(max(0, Q - M * M) / max(N, 1)), 0 where N < 2."""
    with np.errstate(all="ignore"):
        v = Q - M * M
        se = np.sqrt(np.where(v > 0.0, v, 0.0) / np.maximum(N, 1.0)[..., None])
    return np.where((N >= 2.0)[..., None], se, 0.0)


def _mask(tiles, w=W, h=Hh):
    m = np.zeros((h, w), dtype=bool)
    if tiles is None:
        m[:] = True
    else:
        for (x0, y0, tw, th) in tiles:
            m[max(0, y0):max(0, min(h, y0 + th)), max(0, x0):max(0, min(w, x0 + tw))] = True
    return m


def _camera(o, look_at, like):
    cam = _capi.ft_camera.from_buffer_copy(like)                     # keeps up, field of view, aspect ratio and focus
    cam.o = (C.c_double * 3)(*[float(v) for v in o])
    cam.look_at = (C.c_double * 3)(*[float(v) for v in look_at])
    return cam


def _rot_y(v, deg):
    a = H.deg(deg)
    return np.array([math.cos(a) * v[0] + math.sin(a) * v[2], v[1], -math.sin(a) * v[0] + math.cos(a) * v[2]])


def orbit(cam, n, step_deg=1.0):
    """The eye circles the point it looks at, step_deg per call about the y axis."""
    o, look = np.array(cam.o[:]), np.array(cam.look_at[:])
    return [_camera(look + _rot_y(o - look, k * step_deg), look, cam) for k in range(n)]


def dolly(cam, n, step=0.01):
    """The eye moves towards the point it looks at, `step` of the distance per call."""
    o, look = np.array(cam.o[:]), np.array(cam.look_at[:])
    return [_camera(o + k * step * (look - o), look, cam) for k in range(n)]


def pan(cam, n, step_deg=0.3):
    """The eye stays and turns about the y axis."""
    o, look = np.array(cam.o[:]), np.array(cam.look_at[:])
    return [_camera(o, o + _rot_y(look - o, k * step_deg), cam) for k in range(n)]


PATHS = {"orbit": orbit, "dolly": dolly, "pan": pan}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_ft_temporal():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"typedef struct ft_temporal_params\s*\{\s*int32_t max_history, to_frame;\s*double min_normal_dot, position_tolerance_px;\s*\}\s*"
                     r"ft_temporal_params;", hdr)
    assert re.search(r"int32_t ft_temporal_begin\(ft_context\* ctx, int32_t res_h, int32_t res_v, const ft_rect\* tiles, int32_t n_tiles\);", hdr)
    assert re.search(r"int32_t ft_temporal_accumulate\(ft_context\* ctx, const ft_camera\* cam, int32_t spp, const double\* jitter_xy, int32_t sample,\s*"
                     r"uint64_t seed,\s*const ft_temporal_params\* params, int32_t rgba8, void\* out, ft_stats\* stats\);", hdr)
    assert re.search(r"int32_t ft_temporal_fetch\(ft_context\* ctx, double\* mean_rgb, double\* stderr_rgb, double\* length\);", hdr)
    assert re.search(r"int32_t ft_temporal_status\(ft_context\* ctx, int64_t out\[4\]\);", hdr)
    assert re.search(r"int32_t ft_temporal_end\(ft_context\* ctx\);", hdr)
    assert re.search(r"#define FT_TEMPORAL_MIN_WEIGHT 0\.0625\b", hdr) and MIN_WEIGHT == 0.0625
    assert "#define FT_ABI_VERSION 2" in hdr
    lib = C.CDLL(ft.HIP_LIB)
    for name in ("ft_temporal_begin", "ft_temporal_accumulate", "ft_temporal_fetch", "ft_temporal_status", "ft_temporal_end"):
        assert hasattr(lib, name), name
    assert C.sizeof(_capi.ft_temporal_params) == 24
    assert _capi.TEMPORAL_DEFAULTS == dict(max_history=32, to_frame=0, min_normal_dot=0.9, position_tolerance_px=4.0)


def test_arguments_are_checked_in_order_before_the_device():
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    lib, cam = ft.hip_lib(), ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 16 / 9)
    jit = np.zeros((4, 2))

    def call(spp=4, sample=0, null_cam=False, null_params=False, null_jitter=False, **kw):
        p = _capi.ft_temporal_params()
        for k, v in {**_capi.TEMPORAL_DEFAULTS, **kw}.items():
            setattr(p, k, v)
        return lib.ft_temporal_accumulate(ctx._ctx, None if null_cam else C.byref(cam), spp, None if null_jitter else _capi.dptr(jit), sample, 1,
                                          None if null_params else C.byref(p), 0, None, None)

    assert call(spp=0) == -4                                         # corner sampling: no per-sample geometry ray
    assert call(spp=0, sample=9, max_history=0, null_cam=True) == -4  # ... reported before anything else that is wrong
    assert call(sample=4) == -1 and call(sample=-1) == -1            # sample outside [0, spp)
    assert call(spp=-1) == -1 and call(null_jitter=True) == -1
    assert call(null_cam=True) == -1 and call(null_params=True) == -1
    assert call(max_history=0) == -1 and call(max_history=-3) == -1
    assert call(min_normal_dot=float("nan")) == -1 and call(min_normal_dot=1.5) == -1 and call(min_normal_dot=-1.01) == -1
    assert call(position_tolerance_px=0.0) == -1 and call(position_tolerance_px=-1.0) == -1 and call(position_tolerance_px=float("nan")) == -1
    # valid: a host-only context has no device, and that is said before the missing begin (FT_ERR_STATE) could be
    assert call() == -2 and call(sample=3, max_history=1, min_normal_dot=-1.0, to_frame=1) == -2 and call(min_normal_dot=1.0) == -2
    assert lib.ft_temporal_begin(ctx._ctx, 1, 18, None, 0) == -1 and lib.ft_temporal_begin(ctx._ctx, 32, 18, None, 0) == -2
    assert lib.ft_temporal_fetch(ctx._ctx, None, None, None) == -2 and lib.ft_temporal_end(ctx._ctx) == -2
    assert lib.ft_temporal_status(ctx._ctx, (C.c_int64 * 4)()) == -2
    with pytest.raises(ft.FtError) as e:                             # the Python layer sizes its output by the begin
        ctx.temporal_accumulate(cam, 1, jit[:1])
    assert e.value.status == -5
    with pytest.raises(ValueError):
        ctx.temporal_accumulate(cam, 1, jit[:1], history=3)
    ctx.close()


def _flat_inputs(pl, fx, fy, depth=5.0, leaf=0):
    """A surface of leaf `leaf` with the normal -k whose point behind pixel (x, y) projects to (fx[y, x], fy[y, x]) in pl."""
    p = pl["o"] + depth * ray_through_pixel(pl, fx, fy)
    n = np.broadcast_to(-pl["k"], p.shape).copy()
    return p, n, np.full(fx.shape, leaf, dtype=np.int32)


def test_reference_on_hand_worked_cases():
    rng = np.random.default_rng(12)
    h, w = 5, 6
    cam = ft.make_camera((1, 2, -7), (0.5, 0, 3), (0, 1, 0), H.deg(50), 1.3)
    pl = image_plane(cam, w, h)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    on = np.ones((h, w), dtype=bool)
    tight = dict(rtol=1e-12, atol=0)
    p, n, leaf = _flat_inputs(pl, xs, ys)
    frames = [rng.uniform(0.1, 1.0, (h, w, 3)) for _ in range(5)]
    # identical cameras: the running mean, N = k (up to the rounding of the weighted means: fx is an integer only up to a few ulp)
    st, mean, sq = new_state(h, w), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for k, c in enumerate(frames, start=1):
        st = reference(st, pl, c, p, n, leaf, on)
        mean, sq = mean + (c - mean) / k, sq + (c * c - sq) / k
        assert np.allclose(st["M"], mean, **tight) and np.allclose(st["Q"], sq, **tight)
        assert np.allclose(st["N"], k, **tight) and bool(st["history"].all()) == (k > 1) and bool(st["history"].any()) == (k > 1) and not st["taint"].any()
    assert np.array_equal(reference(new_state(h, w), pl, frames[0], p, n, leaf, on)["M"], frames[0])   # the first call: c bit for bit
    # beyond max_history: an exponential average with weight 1 / max_history
    capped = reference(st, pl, frames[0], p, n, leaf, on, max_history=3)
    assert (capped["N"] == 3.0).all() and np.allclose(capped["M"], st["M"] + (frames[0] - st["M"]) / 3.0, **tight)
    # a one-pixel pan: every pixel now shows the point its right-hand neighbour showed, so the history moves one column to the left
    first = reference(new_state(h, w), pl, frames[0], p, n, leaf, on)
    m0 = frames[0]
    p2, _, _ = _flat_inputs(pl, xs + 1.0, ys)
    second = reference(first, pl, frames[1], p2, n, leaf, on)
    assert np.allclose(second["M"][:, :-1], m0[:, 1:] + (frames[1][:, :-1] - m0[:, 1:]) / 2.0, **tight)
    assert np.allclose(second["N"][:, :-1], 2.0, **tight)
    assert (second["N"][:, -1] == 1.0).all() and np.array_equal(second["M"][:, -1], frames[1][:, -1]) and not second["history"][:, -1].any()
    # a tap with another leaf is left out and the rest renormalised: half-way between columns, column 3 belongs to leaf 7
    other = dict(first, leaf=first["leaf"].copy())
    other["leaf"][:, 3] = 7
    p3, _, _ = _flat_inputs(pl, xs + 0.5, ys)
    got = reference(other, pl, frames[1], p3, n, leaf, on)
    assert np.allclose(got["M"][:, 2], m0[:, 2] + (frames[1][:, 2] - m0[:, 2]) / 2.0, **tight)                       # only column 2 (b = 1/2, W = 1/2)
    assert np.allclose(got["M"][:, 3], m0[:, 4] + (frames[1][:, 3] - m0[:, 4]) / 2.0, **tight)                       # only column 4
    both = 0.5 * m0[:, 0] + 0.5 * m0[:, 1]
    assert np.allclose(got["M"][:, 0], both + (frames[1][:, 0] - both) / 2.0, **tight)
    assert got["history"].all() and not got["taint"].any()
    # W < 1/16: the only valid tap (column 4) weighs 0.03, so there is no history; at 0.07 there is
    p4, _, _ = _flat_inputs(pl, np.full((h, w), 3.03), ys)
    none = reference(other, pl, frames[1], p4, n, leaf, on)
    assert (none["N"] == 1.0).all() and np.array_equal(none["M"], frames[1]) and np.array_equal(none["Q"], frames[1] * frames[1]) and not none["history"].any()
    p5, _, _ = _flat_inputs(pl, np.full((h, w), 3.07), ys)
    some = reference(other, pl, frames[1], p5, n, leaf, on)
    assert some["history"].all() and np.allclose(some["M"], m0[:, 4:5] + (frames[1] - m0[:, 4:5]) / 2.0, **tight)
    # a NaN history tap is skipped, a NaN frame pixel stores N = 0 and its NaN, and neither spreads
    bad = dict(first, M=first["M"].copy())
    bad["M"][:, 1, 1] = np.nan
    got = reference(bad, pl, frames[1], p3, n, leaf, on)
    assert np.allclose(got["M"][:, 0], m0[:, 0] + (frames[1][:, 0] - m0[:, 0]) / 2.0, **tight) and np.isfinite(got["M"]).all()
    c = frames[2].copy()
    c[2, 2, 0] = np.nan
    got = reference(first, pl, c, p, n, leaf, on)
    assert got["N"][2, 2] == 0.0 and np.isnan(got["M"][2, 2, 0]) and np.isfinite(np.delete(got["M"].reshape(-1, 3), 2 * w + 2, axis=0)).all()
    after = reference(got, pl, frames[3], p, n, leaf, on)
    assert after["N"][2, 2] == 1.0 and np.isfinite(after["M"]).all() and np.isfinite(after["Q"]).all()
    # pixels outside the tiles neither take nor give, a miss pixel never has history, a surface behind the previous eye (zc <= 0) neither
    tiles = on.copy()
    tiles[:, 4:] = False
    leaf_m = leaf.copy()
    leaf_m[0, :] = -1
    a = reference(new_state(h, w), pl, frames[0], p, n, leaf_m, tiles)
    b = reference(a, pl, frames[1], p, n, leaf_m, tiles)
    assert (b["N"][:, 4:] == 0.0).all() and (b["N"][0, :4] == 1.0).all() and np.array_equal(b["M"][0, :4], frames[1][0, :4])
    assert np.allclose(b["N"][1:, :4], 2.0, **tight)
    behind, _, _ = _flat_inputs(pl, xs, ys, depth=-5.0)
    assert not reference(first, pl, frames[1], behind, n, leaf, on)["history"].any()
    # the standard error of ft_temporal_fetch
    k = len(frames)
    want = np.sqrt((np.mean([f * f for f in frames], axis=0) - np.mean(frames, axis=0) ** 2) / k)
    assert np.allclose(stderr_of(st["M"], st["Q"], st["N"]), want, rtol=1e-9, atol=0) and (stderr_of(first["M"], first["Q"], first["N"]) == 0.0).all()


def test_projection_inverts_ray_through_pixel():
    rng = np.random.default_rng(3)
    for trial in range(200):
        res_h, res_v = int(rng.integers(2, 400)), int(rng.integers(2, 400))
        if trial < 20:
            res_v = res_h + 1 + trial                                # certainly not square
        o = rng.normal(size=3) * 10.0
        cam = ft.make_camera(o, o + rng.normal(size=3) + np.array([0.0, 0.0, 3.0]), (0, 1, 0), H.deg(rng.uniform(5, 120)), rng.uniform(0.5, 2.5))
        pl = image_plane(cam, res_h, res_v)
        x, y = rng.uniform(0, res_h - 1, 64), rng.uniform(0, res_v - 1, 64)
        x[:8], y[:8] = np.round(x[:8]), np.round(y[:8])              # pixel centres sit at integer coordinates
        t = rng.uniform(0.1, 1000.0, 64)
        fx, fy, zc = project(pl, pl["o"] + t[:, None] * ray_through_pixel(pl, x, y))
        assert (zc > 0).all() and np.abs(fx - x).max() < 1e-9 and np.abs(fy - y).max() < 1e-9, (trial, np.abs(fx - x).max(), np.abs(fy - y).max())
    # the pixel size is the reference's: width / (res_v - 1) across, height / (res_h - 1) down
    pl = image_plane(ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 2.0), 160, 90)
    assert math.isclose(pl["pw"], 2.0 * math.tan(H.deg(30)) * 2.0 / 89.0, rel_tol=1e-15) and math.isclose(pl["ph"], 2.0 * math.tan(H.deg(30)) / 159.0, rel_tol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _load(ctx, name, pinhole=False):
    scene = ft.parse_scene_file(H.scene_path(name))
    if pinhole:
        scene.camera.has_focus = 0
    scene.lower(ctx)
    return scene


def _surfaces(ctx, cam, w, h, spp, jit, sample, seed, tiles=None):
    g = ctx.render_aov(cam, w, h, spp, jit, sample=sample, seed=seed, tiles=tiles, channels=["p", "n", "leaf"])
    return g["p"], g["n"], g["leaf"]


def _compare(ctx, st, where, what):
    """The device's M, Q (through the standard error, see the module's docstring) and N against the reference state on the pixels
    `where`.  Returns the worst error in units of the bound, and what ft_temporal_fetch gave."""
    M, se, N = ctx.temporal_fetch()
    mm = st["M"] * st["M"]
    q_seen = se * se * np.maximum(N, 1.0)[..., None] + M * M
    q_want = np.where((st["N"] >= 2.0)[..., None], np.maximum(st["Q"], mm), mm)
    worst = 0.0
    for name, got, want in (("M", M, st["M"]), ("Q", q_seen, q_want), ("N", N, st["N"])):
        g, v = got[where], want[where]
        assert np.array_equal(np.isnan(g), np.isnan(v)), f"{what}: NaN pixels of {name} differ"
        fin = ~np.isnan(v)
        err = np.abs(g[fin] - v[fin]) / (ATOL + RTOL * np.abs(v[fin]))
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert (err <= 1.0).all(), f"{what}: {name} differs by {float(err.max()):.3e} x the bound ({RTOL} relative, {ATOL} absolute) on {int((err > 1.0).sum())} values"
    return worst, M, se, N


# ---------------------------------------------------------------------------------------------------------------- 5. device against reference
@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [None, TILES], ids=["frame", "tiles"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("path", ["orbit", "dolly", "pan"])
@pytest.mark.parametrize("name", ["bunny", "hollow-sphere", "moon", "sample-soft"])
def test_device_matches_the_numpy_restatement(hip, name, path, spp, tiles):
    scene = _load(hip, name)
    cams = PATHS[path](scene.camera, 6)
    jit, sample = ft.jitter_pattern(spp), spp - 1
    inside = _mask(tiles)
    hip.temporal_begin(W, Hh, tiles=tiles)
    st = new_state(Hh, W)
    worst, share, with_history = 0.0, 0.0, []
    for k, cam in enumerate(cams):
        c, _ = hip.render(cam, W, Hh, spp, jit, seed=100 + k)
        p, n, leaf = _surfaces(hip, cam, W, Hh, spp, jit, sample, 100 + k, tiles=tiles)
        out, stats = hip.temporal_accumulate(cam, spp, jit, sample=sample, seed=100 + k, out=np.full((Hh, W, 3), 7.0))
        st = reference(st, image_plane(cam, W, Hh), c, p, n, leaf, inside)
        left_out = int(st["taint"].sum())
        share = max(share, left_out / int(inside.sum()))
        err, M, _, _ = _compare(hip, st, inside & ~st["taint"], f"{name} {path} x{spp} call {k}")
        worst = max(worst, err)
        assert np.array_equal(out[inside], M[inside]) and (out[~inside] == 7.0).all()
        status = hip.temporal_status()
        assert status["calls"] == k + 1 and status["pixels"] == int(inside.sum())
        assert abs(status["with_history"] - int(st["history"].sum())) <= left_out
        assert stats["rays_primary"] == int(inside.sum()) and stats["hits_primary"] == int((leaf[inside] >= 0).sum()) and stats["n_launches"] >= 2
        with_history.append(status["with_history"])
    print(f"temporal parity {name} {path} x{spp} {'tiles' if tiles else 'frame'}: worst error {worst:.3e} x the bound, left out {share:.5%} of the tile pixels, "
          f"pixels with history per call {with_history}")
    assert share <= LEFT_OUT_CAP, f"{share:.5%} of the tile pixels lie within {NEAR} of a threshold"
    assert with_history[0] == 0 and (tiles is not None or min(with_history[1:]) > 0)   # the path does reproject something (the tiles may show no surface)
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 6. static camera
def _footprint_max(a):
    """Per pixel and channel the largest |a| among the pixel and its 8 neighbours: what a bilinear lookup at the pixel's own coordinates,
    right up to rounding, can touch."""
    h, w = a.shape[:2]
    pad = np.zeros((h + 2, w + 2) + a.shape[2:])
    pad[1:-1, 1:-1] = np.abs(a)
    return np.max([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)


@pytest.mark.gpu
def test_static_camera_is_the_running_mean(hip):
    """K = 8 frames of sample-soft (pinhole, so that a pixel's point projects onto the pixel) at 1 spp with 8 seeds.

    What "equal within 1e-12 relative" is relative to: clause 1 returns the pixel's own coordinates only up to the rounding of fx and fy
    (a few 1e-14 of a pixel), so clauses 2 and 3 give a neighbour a weight of that size, and the mean moves by that weight times the
    difference to the neighbour.  A black pixel beside a lit one (the scene has them: measured 5.6e-16 where the running mean is exactly 0)
    cannot agree relative to its own value; the error is held to 1e-12 of the largest value in the pixel's 3x3 footprint, over the calls
    so far and one ring wider with each of them (a neighbour's own error arrives with that weight again, so pixels two away from the
    nearest lit one are no longer exactly black after the sixth call) - the pixel's own value wherever that is the largest.  N is such a
    weighted mean as well: k within 1e-12 relative, not bit for bit (measured: exact up to call 5, 1.5e-16 after).  The standard error is compared as the variance it is the root of: se^2 * N against max(0, Q - M * M) of the test's own
    running means, within 4e-12 of the footprint's largest mean of squares (1e-12 from Q, 2e-12 from M * M as |M| <= sqrt(Q), one more
    for the roundings of the two formulas); se is 0 where N < 2."""
    scene = _load(hip, "sample-soft", pinhole=True)
    cam, jit = scene.camera, np.zeros((1, 2))
    hit = hip.render_aov(cam, W, Hh, 1, jit, channels=["leaf"])["leaf"] >= 0
    hip.temporal_begin(W, Hh)
    mean, sq = np.zeros((Hh, W, 3)), np.zeros((Hh, W, 3))
    scale_m, scale_q = np.zeros((Hh, W, 3)), np.zeros((Hh, W, 3))
    for k in range(1, 9):
        c, _ = hip.render(cam, W, Hh, 1, jit, seed=k)
        out, _ = hip.temporal_accumulate(cam, 1, jit, seed=k)
        mean, sq = mean + (c - mean) / k, sq + (c * c - sq) / k
        scale_m, scale_q = _footprint_max(np.maximum(scale_m, np.abs(mean))), _footprint_max(np.maximum(scale_q, sq))   # one more ring per call
        M, se, N = hip.temporal_fetch()
        lit = hit[..., None] & (scale_m > 0.0)                       # (a footprint that is black throughout must agree exactly: the bound is 0 there)
        err_m = float(np.max(np.abs(M - mean)[lit] / scale_m[lit]))
        err_n = float(np.max(np.abs(N[hit] - k) / k))
        dv = np.abs(se * se * N[..., None] - np.maximum(sq - mean * mean, 0.0))
        err_v = float(np.max(dv[lit] / scale_q[lit]))
        print(f"temporal static camera call {k}: M against the running mean {err_m:.3e} of the footprint's largest value, N against k {err_n:.3e} relative, "
              f"se^2 N against the variance {err_v:.3e} of the footprint's largest mean of squares, largest se {float(se.max()):.4f}")
        assert (np.abs(M - mean)[hit] <= 1e-12 * scale_m[hit]).all() and err_n <= 1e-12
        assert (N[~hit] == 1.0).all() and np.array_equal(M[~hit], c[~hit]) and np.array_equal(out, M)
        assert (se[N < 2.0] == 0.0).all() and (k < 2 or ((dv[hit] <= 4e-12 * scale_q[hit]).all() and se.max() > 0.01))
    assert hip.temporal_status() == {"calls": 8, "pixels": W * Hh, "with_history": int(hit.sum()), "at_max_history": 0}
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 7. it accumulates
@pytest.mark.gpu
def test_orbit_accumulation_is_closer_to_the_converged_frame(hip):
    """A condition, not a measurement: after 12 calls along an orbit of 0.5 degrees per call the accumulated 1-spp frame is closer (RMS)
    to a 256-spp ft_render from the last camera than the raw 1-spp frame of that camera is."""
    scene = _load(hip, "sample-soft", pinhole=True)
    cams = orbit(scene.camera, 12, step_deg=0.5)
    jit = np.zeros((1, 2))
    truth, _ = hip.render(cams[-1], W, Hh, 256, ft.jitter_pattern(256))
    hip.temporal_begin(W, Hh)
    for k, cam in enumerate(cams):
        raw, _ = hip.render(cam, W, Hh, 1, jit, seed=k + 1)
        got, _ = hip.temporal_accumulate(cam, 1, jit, seed=k + 1, to_frame=1)
    status = hip.temporal_status()
    filtered, _ = hip.denoise(cams[-1], W, Hh, 1, jit, seed=12, iterations=4, sigma_colour=1.0, sigma_normal=0.3, sigma_position=0.0, demodulate=1)
    rms = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    print(f"temporal sample-soft orbit, 12 calls at 1 spp against 256 spp: RMS raw {rms(raw):.5f}, accumulated {rms(got):.5f} (ratio {rms(got) / rms(raw):.3f}), "
          f"accumulated + ft_denoise {rms(filtered):.5f} (ratio {rms(filtered) / rms(raw):.3f}); {status['with_history']} of {status['pixels']} pixels with history")
    assert rms(got) < rms(raw)
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 8. disocclusion
@pytest.mark.gpu
def test_disoccluded_and_miss_pixels_start_again(hip):
    scene = _load(hip, "bunny")
    jit = np.zeros((1, 2))
    o, look = np.array(scene.camera.o[:]), np.array(scene.camera.look_at[:])
    cams = orbit(scene.camera, 3) + [_camera(look + _rot_y(o - look, 180.0), look, scene.camera)]   # ... then a jump to the opposite side
    hip.temporal_begin(W, Hh)
    for k, cam in enumerate(cams):
        c, _ = hip.render(cam, W, Hh, 1, jit, seed=k)
        miss = hip.render_aov(cam, W, Hh, 1, jit, seed=k, channels=["leaf"])["leaf"] < 0
        hip.temporal_accumulate(cam, 1, jit, seed=k, fetch=False)
        M, _, N = hip.temporal_fetch()
        status = hip.temporal_status()
        fresh = N == 1.0
        assert miss.any() and fresh[miss].all() and np.array_equal(M[miss], c[miss])
        assert np.isfinite(c).all() and int(fresh.sum()) == status["pixels"] - status["with_history"] and (N[~fresh] >= 2.0).all()
        assert np.array_equal(M[fresh], c[fresh])
        print(f"temporal disocclusion call {k}: {status['with_history']} of {status['pixels']} pixels with history, {int((~miss).sum())} hit pixels")
    assert status["with_history"] < int((~miss).sum())               # the jump did lose surfaces
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 9. output forms
@pytest.mark.gpu
def test_output_forms(hip):
    scene = _load(hip, "moon")
    cams, jit = orbit(scene.camera, 3, step_deg=0.2), ft.jitter_pattern(2)
    tiles = TILES + [(-5, 60, 30, 12)]                               # one rect clipped by the frame
    inside = _mask(tiles)
    for to_frame in (0, 1):
        hip.temporal_begin(W, Hh, tiles=tiles)
        twin = ft.Context(device=0)                                  # the same sequence, asked for bytes
        try:
            scene.lower(twin)
            twin.temporal_begin(W, Hh, tiles=tiles)
            for k, cam in enumerate(cams):
                c, _ = hip.render(cam, W, Hh, 2, jit, seed=k)
                twin.render(cam, W, Hh, 2, jit, seed=k, fetch=False)
                f64, _ = hip.temporal_accumulate(cam, 2, jit, seed=k, to_frame=to_frame, out=np.full((Hh, W, 3), 7.0))
                u8, _ = twin.temporal_accumulate(cam, 2, jit, seed=k, rgba8=True, out=np.full((Hh, W, 4), 9, dtype=np.uint8))
                assert np.array_equal(u8[inside], ft.quantise_rgba8(f64)[inside]) and (u8[~inside] == 9).all() and (f64[~inside] == 7.0).all()
                frame = hip.fetch_frame(np.zeros((Hh, W, 3)))
                if to_frame:
                    assert np.array_equal(frame[inside], f64[inside]) and np.array_equal(frame[~inside], c[~inside])
                else:
                    assert np.array_equal(frame, c)
                M, _, N = hip.temporal_fetch()
                assert np.array_equal(M[inside], f64[inside]) and (N[~inside] == 0.0).all() and (M[~inside] == 0.0).all()
            assert not np.array_equal(f64[inside], c[inside])        # it blended something
        finally:
            twin.close()
        with ft.PinnedArray((Hh, W, 3)) as pinned:
            hip.render(cams[-1], W, Hh, 2, jit, seed=9, fetch=False)
            hip.temporal_accumulate(cams[-1], 2, jit, seed=9, out=pinned)
            assert np.array_equal(pinned[inside], hip.temporal_fetch()[0][inside])
        hip.temporal_end()
    with pytest.raises(ft.FtError) as e:
        hip.temporal_fetch()
    assert e.value.status == -5


# ---------------------------------------------------------------------------------------------------------------- 10. nothing existing changes
@pytest.mark.gpu
def test_everything_else_is_left_alone(hip):
    scene = _load(hip, "sample-soft")
    cam, jit = scene.camera, ft.jitter_pattern(4)
    cams = orbit(cam, 3)
    w, h = W - W % 8, Hh - Hh % 8                                    # an adaptive progressive accumulation needs whole 8x8 blocks
    first, _ = hip.render(cam, w, h, 4, jit, seed=11)
    hip.progressive_begin(cam, w, h, tolerance=0.01, min_samples=2)
    for k in range(3):
        hip.progressive_pass(2, ft.jitter_pattern(2, seed=k + 1), seed=k)
    mean, se, samples = hip.progressive_fetch()
    for to_frame in (0, 1):
        hip.temporal_begin(w, h)
        for k, c in enumerate(cams):
            hip.render(c, w, h, 4, jit, seed=k, fetch=False)
            hip.temporal_accumulate(c, 4, jit, sample=1, seed=k, to_frame=to_frame, fetch=False)
        assert hip.temporal_status()["with_history"] > 0
        again, _ = hip.render(cam, w, h, 4, jit, seed=11)
        assert np.array_equal(again, first)
        hip.render(cam, w, h, 4, jit, seed=11, fetch=False)          # ... and once more, straight after a frame of the same signature
        assert np.array_equal(hip.fetch_frame(np.zeros((h, w, 3))), first)
    mean2, se2, samples2 = hip.progressive_fetch()
    assert np.array_equal(mean, mean2) and np.array_equal(se, se2) and np.array_equal(samples, samples2)
    hip.progressive_end()
    # a second begin replaces the first: no history behind the next call
    hip.render(cam, w, h, 4, jit, seed=1, fetch=False)
    hip.temporal_begin(w, h)
    assert hip.temporal_status() == {"calls": 0, "pixels": w * h, "with_history": 0, "at_max_history": 0}
    hip.temporal_accumulate(cam, 4, jit, seed=1, fetch=False)
    assert hip.temporal_status()["with_history"] == 0 and hip.temporal_status()["calls"] == 1
    # state errors: another frame size, an RGBA8 frame, a caller's commit
    hip.render(cam, W, Hh, 4, jit, fetch=False)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_accumulate(cam, 4, jit)
    assert e.value.status == -5
    hip.render_rgba8(cam, w, h, 4, jit, fetch=False)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_accumulate(cam, 4, jit)
    assert e.value.status == -5
    hip.render(cam, w, h, 4, jit, fetch=False)
    hip.temporal_accumulate(cam, 4, jit, fetch=False)
    assert hip.temporal_status()["calls"] == 2                       # the failed calls left the accumulation as it was
    hip.commit()
    hip.render(cam, w, h, 4, jit, fetch=False)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_accumulate(cam, 4, jit)
    assert e.value.status == -5 and "ft_temporal_begin" in str(e.value)
    fresh = ft.Context(device=0)
    try:
        scene.lower(fresh)
        fresh.temporal_begin(W, Hh)
        with pytest.raises(ft.FtError) as e:
            fresh.temporal_accumulate(cam, 4, jit)
        assert e.value.status == -5                                  # nothing rendered yet
    finally:
        fresh.close()
    two = ft.Context(device=[0, 0])
    try:
        scene.lower(two)
        with pytest.raises(ft.FtError) as e:
            two.temporal_begin(W, Hh)
        assert e.value.status == -4 and "bands" in str(e.value)
    finally:
        two.close()


# ---------------------------------------------------------------------------------------------------------------- 11. NaN
@pytest.mark.gpu
def test_non_finite_pixels_stay_where_they_are(hip, golden):
    """The scene with which test_denoise.py produces its NaN frame (a negative base under a fractional exponent, Shading.fs:85-87)."""
    case = [c for c in golden["hand_derived_shading"]["cases"] if c["name"] == "specular_negative_base_fractional_exponent_is_nan"][0]
    H.build_described_scene(hip, case["objects"], case["lights"])
    cams = orbit(ft.make_camera((0, 0, -3), (0, 0, 0), (0, 1, 0), H.deg(40.0), 1.0), 3)
    jit = np.zeros((1, 2))
    hip.temporal_begin(64, 64)
    st = new_state(64, 64)
    everywhere = _mask(None, 64, 64)
    for k, cam in enumerate(cams):
        raw, _ = hip.render(cam, 64, 64, 1, jit)
        bad = np.isnan(raw).any(-1)
        assert bad.any() and not bad.all()
        p, n, leaf = _surfaces(hip, cam, 64, 64, 1, jit, 0, ft.DEFAULT_SEED)
        out, _ = hip.temporal_accumulate(cam, 1, jit)
        st = reference(st, image_plane(cam, 64, 64), raw, p, n, leaf, everywhere)
        assert int(st["taint"].sum()) <= LEFT_OUT_CAP * 64 * 64
        _, M, _, N = _compare(hip, st, everywhere & ~st["taint"], f"NaN frame call {k}")
        assert np.array_equal(~np.isfinite(M).all(-1), bad) and (N[bad] == 0.0).all() and (N[~bad] >= 1.0).all()
        assert np.array_equal(np.isnan(out), np.isnan(M))
    assert hip.temporal_status()["with_history"] > 0
    hip.temporal_end()

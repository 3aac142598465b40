"""ft_temporal_filter (Context.temporal_filter): the history set the last ft_temporal_accumulate wrote, filtered on the device by an
edge-avoiding a-trous filter whose colour term is scaled by a per-pixel variance that is filtered from iteration to iteration.
`reference` below restates the definition of include/functracer_hip.h / DESIGN.md 13 in numpy; its inputs come from the public API
(temporal_fetch for M, the standard error and N; render_aov with the last accumulate's arguments for p, n, leaf and colour, which are
bit-identical to what the set holds by clause 6 of ft_temporal_accumulate), so it shares no code with the kernels.

The GPU tests print the figures they assert on; what an MI355X gave is in DESIGN.md 13 "Measured"."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import helpers as H
from .test_denoise import KERNEL, TILES, _shift
from .test_temporal import PATHS, _load, _mask, orbit

W, Hh = 160, 90
KERNEL3 = np.array([1 / 4, 1 / 2, 1 / 4])
PARAMS = dict(sigma_colour=2.0, sigma_normal=0.3, sigma_position=1.0, albedo_floor=1e-3, variance_floor=1e-6)
# test_it_denoises: chosen on the GPU among the 900 combinations DESIGN.md 13 lists, then fixed
DENOISE_PARAMS = dict(iterations=2, demodulate=0, min_history=4, sigma_colour=8.0, sigma_normal=0.1, sigma_position=0.0, albedo_floor=1e-3, variance_floor=1e-6)


# ---------------------------------------------------------------------------------------------------------------- the definition, in numpy
def _sq(a):
    return a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]


def reference(M, se, N, n, p, hit, in_tiles, a=None, match=None, iterations=4, demodulate=1, min_history=4, sigma_colour=2.0, sigma_normal=0.3,
              sigma_position=0.0, albedo_floor=1e-3, variance_floor=1e-6):
    """(u_N * d, v_N, v_0) for the pixels of `in_tiles` (elsewhere 0).  M, se, n, p, a: [h, w, 3]; N: [h, w]; hit (the set's leaf >= 0),
    in_tiles, match (the guide's leaf equals the set's; None: everywhere): [h, w] bool."""
    cls = np.where(in_tiles, hit.astype(np.int8), 2)
    d = np.ones_like(M)
    if demodulate:
        same = hit if match is None else hit & match
        d = np.where(same[..., None], np.where(a > albedo_floor, a, albedo_floor), 1.0)
    with np.errstate(all="ignore"):
        u = M / d
        r = se / d
        vt = (1.0 / 3.0) * _sq(r)
        # the spatial estimate, used where the history is short
        sg, s1, s2 = np.zeros(N.shape), np.zeros_like(M), np.zeros_like(M)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                cq, uq = _shift(cls, dy, dx, 2), _shift(u, dy, dx, np.nan)
                E = np.zeros(N.shape)
                if sigma_normal > 0:
                    E = E + _sq(n - _shift(n, dy, dx, 0.0)) / sigma_normal ** 2
                if sigma_position > 0:
                    E = E + _sq(p - _shift(p, dy, dx, 0.0)) / sigma_position ** 2
                E = np.where(hit, E, 0.0)                            # a miss pixel has no geometric term
                take = (cq == cls) & (cls != 2) & np.isfinite(uq).all(-1)
                g = np.where(take, np.exp(-E), 0.0)
                sg = sg + g
                s1 = s1 + np.where(take[..., None], g[..., None] * uq, 0.0)
                s2 = s2 + np.where(take[..., None], g[..., None] * (uq * uq), 0.0)
        m1, m2 = s1 / sg[..., None], s2 / sg[..., None]
        var = m2 - m1 * m1
        vs = (1.0 / 3.0) * np.where(var > 0.0, var, 0.0).sum(-1)
        v = np.where((N < min_history) & (vs > vt), vs, vt)
        v0 = np.where(in_tiles, v, 0.0)
        if iterations == 0:
            return np.where(in_tiles[..., None], M, 0.0), v0, v0     # M bit for bit: no division and multiplication by d
        for i in range(iterations):
            s = 2 ** i
            gs, gw = np.zeros(N.shape), np.zeros(N.shape)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    cq, vq = _shift(cls, dy, dx, 2), _shift(v, dy, dx, np.nan)
                    take = (cq == cls) & np.isfinite(vq)
                    wgt = KERNEL3[dx + 1] * KERNEL3[dy + 1]
                    gs = gs + np.where(take, wgt * vq, 0.0)
                    gw = gw + np.where(take, wgt, 0.0)
            gv = gs / gw
            num, den, vnum = np.zeros_like(u), np.zeros(N.shape), np.zeros(N.shape)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, uq, vq = _shift(cls, s * dy, s * dx, 2), _shift(u, s * dy, s * dx, np.nan), _shift(v, s * dy, s * dx, np.nan)
                    E = np.zeros(N.shape)
                    if sigma_normal > 0:
                        E = E + _sq(n - _shift(n, s * dy, s * dx, 0.0)) / sigma_normal ** 2
                    if sigma_position > 0:
                        E = E + _sq(p - _shift(p, s * dy, s * dx, 0.0)) / sigma_position ** 2
                    E = np.where(hit, E, 0.0)
                    if sigma_colour > 0:
                        E = E + _sq(u - uq) / (sigma_colour ** 2 * (gv + variance_floor))
                    take = (cq == cls) & (cls != 2) & np.isfinite(uq).all(-1) & np.isfinite(vq) & ~np.isnan(E)
                    wgt = np.where(take, KERNEL[dx + 2] * KERNEL[dy + 2] * np.exp(-E), 0.0)
                    num = num + np.where(take[..., None], wgt[..., None] * uq, 0.0)
                    den = den + wgt
                    vnum = vnum + np.where(take, wgt * wgt * vq, 0.0)
            own = np.isfinite(u).all(-1) & np.isfinite(v) & (cls != 2)
            u = np.where(own[..., None], num / den[..., None], u)
            v = np.where(own, vnum / (den * den), v)
        return np.where(in_tiles[..., None], u * d, 0.0), np.where(in_tiles, v, 0.0), v0


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_ft_temporal_filter():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"typedef struct ft_temporal_filter_params\s*\{\s*int32_t iterations, demodulate, min_history, to_frame;\s*"
                     r"double sigma_colour, sigma_normal, sigma_position, albedo_floor, variance_floor;\s*\}\s*ft_temporal_filter_params;", hdr)
    assert re.search(r"int32_t ft_temporal_filter\(ft_context\* ctx, const ft_camera\* cam, int32_t spp, const double\* jitter_xy, int32_t sample, uint64_t seed,\s*"
                     r"const ft_temporal_filter_params\* params, int32_t rgba8, void\* out, double\* out_variance, ft_stats\* stats\);", hdr)
    assert "#define FT_ABI_VERSION 2" in hdr
    assert hasattr(C.CDLL(ft.HIP_LIB), "ft_temporal_filter")
    assert C.sizeof(_capi.ft_temporal_filter_params) == 56
    assert set(_capi.TEMPORAL_FILTER_DEFAULTS) == {f for f, _ in _capi.ft_temporal_filter_params._fields_}


def test_arguments_are_checked_in_order_before_the_device():
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    lib, cam = ft.hip_lib(), ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 16 / 9)
    out, var, jit = np.zeros((18, 32, 3)), np.zeros((18, 32)), np.zeros((4, 2))

    def call(spp=4, sample=0, out=out, var=None, null_cam=False, null_params=False, null_jitter=False, **kw):
        p = _capi.ft_temporal_filter_params()
        for k, v in {**_capi.TEMPORAL_FILTER_DEFAULTS, **kw}.items():
            setattr(p, k, v)
        return lib.ft_temporal_filter(ctx._ctx, None if null_cam else C.byref(cam), spp, None if null_jitter else _capi.dptr(jit), sample, 1,
                                      None if null_params else C.byref(p), 0, out.ctypes.data_as(C.c_void_p) if out is not None else None,
                                      _capi.dptr(var) if var is not None else None, None)

    nan = float("nan")
    # 1. null params, or neither output - before anything else that is wrong
    assert call(null_params=True) == -1 and call(out=None) == -1 and call(out=None, spp=0, iterations=9) == -1
    assert call(out=None, var=var) == -2                             # the variance alone is an output
    # 2. the parameters - before corner sampling is refused
    assert call(iterations=-1) == -1 and call(iterations=7) == -1 and call(iterations=7, spp=0) == -1
    assert call(sigma_colour=-0.1) == -1 and call(sigma_normal=-1.0) == -1 and call(sigma_position=-1e-9) == -1 and call(sigma_normal=nan) == -1
    assert call(min_history=0) == -1 and call(min_history=-2, spp=0) == -1
    assert call(variance_floor=0.0) == -1 and call(variance_floor=-1.0) == -1 and call(variance_floor=nan) == -1 and call(variance_floor=0.0, demodulate=0) == -1
    assert call(demodulate=1, albedo_floor=0.0) == -1 and call(demodulate=1, albedo_floor=nan, spp=0) == -1 and call(demodulate=0, albedo_floor=0.0) == -2
    # 3. with demodulate, the guide sample's checks: corner sampling first
    assert call(spp=0) == -4 and call(spp=0, sample=9, null_cam=True, null_jitter=True) == -4
    assert call(sample=4) == -1 and call(sample=-1) == -1 and call(spp=-1) == -1 and call(null_jitter=True) == -1 and call(null_cam=True) == -1
    # ... none of which is read without demodulate
    assert call(demodulate=0, spp=0, sample=9, null_cam=True, null_jitter=True) == -2
    # 4. valid: a host-only context has no device, and that is said before the missing begin (FT_ERR_STATE) could be
    assert call() == -2 and call(iterations=0) == -2 and call(iterations=6, sample=3, to_frame=1, min_history=1) == -2
    with pytest.raises(ft.FtError) as e:                             # the Python layer sizes its output by the begin
        ctx.temporal_filter(cam, 1, jit[:1])
    assert e.value.status == -5
    ctx._temporal = (32, 18)
    with pytest.raises(ValueError):
        ctx.temporal_filter(cam, 1, jit[:1], sigma=1.0)
    with pytest.raises(ft.FtError) as e:
        ctx.temporal_filter(demodulate=0)
    assert e.value.status == -2
    ctx._temporal = None
    ctx.close()


def test_reference_on_hand_worked_cases():
    rng = np.random.default_rng(7)
    h, w = 9, 11
    on, z3 = np.ones((h, w), dtype=bool), np.zeros((h, w, 3))
    flat_n = np.zeros((h, w, 3))
    flat_n[..., 2] = 1.0
    long_n = np.full((h, w), 8.0)
    # a constant image with a constant variance on one flat surface: every E is 0, so interior pixels keep u, and
    # v_1 = v * sum (h h)^2 / (sum h h)^2 = v * (sum h^2)^2 = v * (70 / 256)^2 = v * (35 / 128)^2
    var = 0.04
    M, se = np.full((h, w, 3), 0.375), np.full((h, w, 3), np.sqrt(var))
    got, v1, v0 = reference(M, se, long_n, flat_n, z3, on, on, iterations=1, demodulate=0)
    assert np.allclose(v0, var, rtol=1e-15, atol=0) and np.allclose(got, 0.375, rtol=1e-15, atol=0)
    assert np.allclose(v1[2:-2, 2:-2], var * (35.0 / 128.0) ** 2, rtol=1e-14, atol=0)
    assert (v1[0, 0] > v1[4, 5]) and np.isclose(np.sum(KERNEL ** 2), 70.0 / 256.0, rtol=1e-15)   # fewer taps at the corner: less averaging
    # ... and with demodulation by a constant albedo of 1/2 the variance of u is four times the variance of M
    _, _, v0d = reference(M, se, long_n, flat_n, z3, on, on, a=np.full((h, w, 3), 0.5), iterations=1, demodulate=1)
    assert np.allclose(v0d, 4.0 * var, rtol=1e-14, atol=0)
    # a guide leaf that is not the set's leaf gives d = 1 there
    match = on.copy()
    match[4, 5] = False
    _, _, v0m = reference(M, se, long_n, flat_n, z3, on, on, a=np.full((h, w, 3), 0.5), match=match, iterations=1, demodulate=1)
    assert np.isclose(v0m[4, 5], var, rtol=1e-14) and np.isclose(v0m[4, 4], 4.0 * var, rtol=1e-14)
    # two regions with opposite normals, sigma_normal small: |n - n'|^2 / sigma^2 = 4 / 1e-4, exp(-40000) underflows to 0 (test_denoise.py's
    # argument), so each region is filtered on its own and (being constant) keeps its value; without the normal term the edge bleeds
    M = np.zeros((h, w, 3))
    M[:, :5], M[:, 5:] = 0.2, 0.9
    n2 = np.zeros((h, w, 3))
    n2[:, :5, 2], n2[:, 5:, 2] = 1.0, -1.0
    kept, _, _ = reference(M, z3, long_n, n2, z3, on, on, iterations=2, sigma_colour=0.0, sigma_normal=0.01, demodulate=0)
    assert np.allclose(kept, M, rtol=1e-15, atol=0)
    bled, _, _ = reference(M, z3, long_n, n2, z3, on, on, iterations=2, sigma_colour=0.0, sigma_normal=0.0, demodulate=0)
    assert 0.2 < bled[4, 4, 0] < bled[4, 5, 0] < 0.9
    # a pixel with N < min_history between noisy neighbours takes the spatial estimate, one with N >= min_history does not
    M = rng.uniform(0.0, 1.0, (h, w, 3))
    N = np.full((h, w), 4.0)
    N[4, 5] = 3.0
    se = np.full((h, w, 3), 1e-3)
    _, _, v0 = reference(M, se, N, flat_n, z3, on, on, iterations=1, demodulate=0, min_history=4, sigma_normal=0.0)
    win = M[1:8, 2:9].reshape(-1, 3)
    want = np.mean(np.maximum((win * win).mean(0) - win.mean(0) ** 2, 0.0))
    assert np.isclose(v0[4, 5], want, rtol=1e-12) and v0[4, 5] > 1e-3
    assert np.allclose(np.delete(v0.reshape(-1), 4 * w + 5), 1e-6, rtol=1e-12, atol=0)
    _, _, v0 = reference(M, se, N, flat_n, z3, on, on, iterations=1, demodulate=0, min_history=3, sigma_normal=0.0)
    assert np.allclose(v0, 1e-6, rtol=1e-12, atol=0)
    # the larger of the two: a temporal variance above the spatial one stays
    se_big = np.full((h, w, 3), 10.0)
    _, _, v0 = reference(M, se_big, N, flat_n, z3, on, on, iterations=1, demodulate=0, min_history=4, sigma_normal=0.0)
    assert np.allclose(v0, 100.0, rtol=1e-14, atol=0)
    # a NaN pixel (N = 0, as clause 5 of ft_temporal_accumulate stores it) stays NaN, u and v pass through, and its neighbours stay finite
    Mn, Nn = M.copy(), np.full((h, w), 8.0)
    Mn[3, 3, 1], Nn[3, 3] = np.nan, 0.0
    got, vN, v0 = reference(Mn, se, Nn, flat_n, z3, on, on, iterations=3, demodulate=0)
    assert np.isnan(got[3, 3, 1]) and np.array_equal(got[3, 3, ::2], Mn[3, 3, ::2]) and vN[3, 3] == v0[3, 3]
    assert np.isfinite(np.delete(got.reshape(-1, 3), 3 * w + 3, axis=0)).all() and np.isfinite(vN).all()
    # classes never mix and pixels outside the tiles neither give nor take
    hit = np.zeros((h, w), dtype=bool)
    hit[:, :4] = True
    tiles = on.copy()
    tiles[:, 8:] = False
    got, vN, _ = reference(M, se, long_n, z3, z3, hit, tiles, iterations=2, sigma_colour=0.0, demodulate=0)
    assert (got[:, 8:] == 0.0).all() and (vN[:, 8:] == 0.0).all()
    assert got[:, :4].min() >= M[:, :4].min() and got[:, :4].max() <= M[:, :4].max()
    assert got[:, 4:8].min() >= M[:, 4:8].min() and got[:, 4:8].max() <= M[:, 4:8].max()
    # iterations = 0: M bit for bit, with and without demodulation, and v_0
    for demodulate in (0, 1):
        got, vN, v0 = reference(M, se, N, flat_n, z3, on, on, a=np.full((h, w, 3), 0.3), iterations=0, demodulate=demodulate)
        assert np.array_equal(got, M) and np.array_equal(vN, v0)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _inputs(ctx, cam, spp, jit, sample, seed, tiles=None, w=W, h=Hh):
    """What the restatement is fed with, through the public API only."""
    M, se, N = ctx.temporal_fetch()
    g = ctx.render_aov(cam, w, h, spp, jit, sample=sample, seed=seed, tiles=tiles, channels=["n", "p", "colour", "leaf"])
    return M, se, N, g["n"], g["p"], g["leaf"] >= 0, g["colour"]


def _compare(got, got_v, want, want_v, v0, mask, what):
    """The result relative to the largest value of the plane (the contract 1e-4 and 1e-6), the variance relative to the largest v_0 of
    the case (1e-6).  No pixel is left out."""
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got_v), np.isnan(want_v)), f"{what}: NaN pixels differ"
    fin = ~np.isnan(want)
    scale = float(np.abs(want[fin & mask[..., None]]).max())
    err = float((np.abs(got - want)[fin & mask[..., None]]).max() / scale) if scale > 0 else float(np.abs(got - want)[fin & mask[..., None]].max())
    vscale = float(v0[mask & np.isfinite(v0)].max())
    finv = ~np.isnan(want_v) & mask
    verr = float(np.abs(got_v - want_v)[finv].max() / vscale) if vscale > 0 else float(np.abs(got_v - want_v)[finv].max())
    print(f"temporal filter parity {what}: result {err:.3e} of the plane's largest value, variance {verr:.3e} of the largest v_0 ({vscale:.3e})")
    assert err < H.PIXEL_RTOL and err < 1e-6, f"{what}: result differs by {err:.3e} of the plane's largest value"
    assert verr < 1e-6, f"{what}: variance differs by {verr:.3e} of the largest v_0"
    return err, verr


# ---------------------------------------------------------------------------------------------------------------- 1. device against reference
@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [None, TILES], ids=["frame", "tiles"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("path", ["orbit", "dolly", "pan"])
@pytest.mark.parametrize("name", ["bunny", "hollow-sphere", "moon", "sample-soft"])
def test_device_matches_the_numpy_restatement(hip, name, path, spp, tiles):
    scene = _load(hip, name)
    cams = PATHS[path](scene.camera, 4)
    jit, sample = ft.jitter_pattern(spp), spp - 1
    inside = _mask(tiles)
    hip.temporal_begin(W, Hh, tiles=tiles)
    worst = [0.0, 0.0]
    for k, cam in enumerate(cams):
        hip.render(cam, W, Hh, spp, jit, seed=100 + k, fetch=False)
        hip.temporal_accumulate(cam, spp, jit, sample=sample, seed=100 + k, fetch=False)
        if k == 0:                                                   # N = 1 everywhere: every tile pixel takes the spatial path
            combos = [(3, 1, 4)]
        elif k == len(cams) - 1:
            combos = [(it, dm, mh) for it in (1, 3, 5) for dm in (0, 1) for mh in (2, 4)]
        else:
            continue
        M, se, N, n, p, hit, a = _inputs(hip, cam, spp, jit, sample, 100 + k, tiles=tiles)
        for iterations, demodulate, min_history in combos:
            kw = dict(PARAMS, iterations=iterations, demodulate=demodulate, min_history=min_history)
            got, got_v, st = hip.temporal_filter(cam, spp, jit, sample=sample, seed=100 + k, out=np.full((Hh, W, 3), 7.0), variance=np.full((Hh, W), 5.0), **kw)
            want, want_v, v0 = reference(M, se, N, n, p, hit, inside, a=a, **kw)
            assert (got[~inside] == 7.0).all() and (got_v[~inside] == 5.0).all()
            e, ev = _compare(got, got_v, want, want_v, v0, inside, f"{name} {path} x{spp} {'tiles' if tiles else 'frame'} call {k} N={iterations} demodulate={demodulate} min_history={min_history}")
            worst = [max(worst[0], e), max(worst[1], ev)]
            assert st["rays_primary"] == (int(inside.sum()) if demodulate else 0) and st["n_launches"] >= iterations + 1 + demodulate
            assert (st["trace_kernel_ms"] > 0) == bool(demodulate) and st["kernel_ms"] > st["trace_kernel_ms"]
            if tiles is None:
                assert not np.array_equal(got, M)                    # it filtered something
    print(f"temporal filter parity {name} {path} x{spp} {'tiles' if tiles else 'frame'}: worst result error {worst[0]:.3e}, worst variance error {worst[1]:.3e}")
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 2. the variance steers
def _orbit_run(ctx, scene, calls, to_frame=1, step_deg=0.5):
    cams, jit = orbit(scene.camera, calls, step_deg=step_deg), np.zeros((1, 2))
    ctx.temporal_begin(W, Hh)
    for k, cam in enumerate(cams):
        raw, _ = ctx.render(cam, W, Hh, 1, jit, seed=k + 1)
        acc, _ = ctx.temporal_accumulate(cam, 1, jit, seed=k + 1, to_frame=to_frame)
    return cams[-1], jit, calls, raw, acc                            # (the last call's seed is `calls`)


@pytest.mark.gpu
def test_the_variance_steers_the_filter(hip):
    scene = _load(hip, "sample-soft", pinhole=True)
    cam, jit, seed, _, acc = _orbit_run(hip, scene, 6)
    kw = dict(iterations=4, demodulate=1, min_history=4, sigma_colour=1.0, sigma_normal=0.3, sigma_position=0.0, albedo_floor=1e-3)
    got, var, _ = hip.temporal_filter(cam, 1, jit, seed=seed, variance=True, variance_floor=1e-6, **kw)
    geometric, _, _ = hip.temporal_filter(cam, 1, jit, seed=seed, variance_floor=1e30, **kw)   # the colour term vanishes: purely geometric
    denoised, _ = hip.denoise(cam, W, Hh, 1, jit, seed=seed, iterations=4, demodulate=1, sigma_colour=1.0, sigma_normal=0.3, sigma_position=0.0, albedo_floor=1e-3)
    scale = float(np.abs(got).max())
    d_geo, d_den = float(np.abs(got - geometric).max()) / scale, float(np.abs(got - denoised).max()) / scale
    print(f"temporal filter steering, sample-soft after 6 orbit calls: against variance_floor 1e30 {d_geo:.3e}, against ft_denoise on the to_frame frame {d_den:.3e} "
          f"(largest difference over the plane's largest value); variance {float(var.min()):.3e} .. {float(var.max()):.3e}")
    assert not np.allclose(got, geometric, rtol=1e-6, atol=0) and d_geo > 1e-6
    assert not np.allclose(got, denoised, rtol=1e-6, atol=0) and d_den > 1e-6
    assert not np.array_equal(got, acc) and var.max() > 0 and (var >= 0).all()
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 3. it denoises
@pytest.mark.gpu
def test_it_denoises(hip):
    """DESIGN.md 12's setup: sample-soft (pinhole), 1 spp, an orbit of 0.5 degrees per call, 12 calls, RMS error against a 256-spp
    ft_render from the last camera.  (a) the accumulated frame, (b) ft_denoise on top of it with section 12's parameters, (c)
    ft_temporal_filter with DENOISE_PARAMS.  The run is seeded and deterministic: (c) < (b) and (c) < (a), no noise margin."""
    scene = _load(hip, "sample-soft", pinhole=True)
    truth, _ = hip.render(orbit(scene.camera, 12, step_deg=0.5)[-1], W, Hh, 256, ft.jitter_pattern(256))
    cam, jit, seed, raw, acc = _orbit_run(hip, scene, 12)
    on_top, _ = hip.denoise(cam, W, Hh, 1, jit, seed=seed, iterations=4, sigma_colour=1.0, sigma_normal=0.3, sigma_position=0.0, demodulate=1)
    got, _, _ = hip.temporal_filter(cam, 1, jit, seed=seed, **DENOISE_PARAMS)
    rms = lambda x: float(np.sqrt(np.mean((x - truth) ** 2)))
    a, b, c = rms(acc), rms(on_top), rms(got)
    print(f"temporal filter sample-soft orbit, 12 calls at 1 spp against 256 spp: RMS raw {rms(raw):.5f}, (a) accumulated {a:.5f}, (b) ft_denoise on top {b:.5f}, "
          f"(c) ft_temporal_filter {c:.5f} with {DENOISE_PARAMS}")
    assert c < b
    assert c < a
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 4. output forms
@pytest.mark.gpu
def test_output_forms(hip):
    scene = _load(hip, "moon")
    cams, jit = orbit(scene.camera, 3, step_deg=0.2), ft.jitter_pattern(2)
    tiles = TILES + [(-5, 60, 30, 12)]                               # one rect clipped by the frame
    inside = _mask(tiles)
    hip.temporal_begin(W, Hh, tiles=tiles)
    for k, cam in enumerate(cams):
        c, _ = hip.render(cam, W, Hh, 2, jit, seed=k)
        hip.temporal_accumulate(cam, 2, jit, seed=k, fetch=False)
    M, _, _ = hip.temporal_fetch()
    args = dict(spp=2, jitter=jit, seed=2)
    for iterations in (0, 3):
        for demodulate in (0, 1):
            kw = dict(iterations=iterations, demodulate=demodulate)
            f64, var, _ = hip.temporal_filter(cams[-1], out=np.full((Hh, W, 3), 7.0), variance=np.full((Hh, W), 5.0), **args, **kw)
            u8, _, _ = hip.temporal_filter(cams[-1], rgba8=True, out=np.full((Hh, W, 4), 9, dtype=np.uint8), **args, **kw)
            assert np.array_equal(u8[inside], ft.quantise_rgba8(f64)[inside]) and (u8[~inside] == 9).all()
            assert (f64[~inside] == 7.0).all() and (var[~inside] == 5.0).all() and np.isfinite(var[inside]).all()
            assert np.array_equal(f64[inside], M[inside]) == (iterations == 0)
            none, only_var, _ = hip.temporal_filter(cams[-1], out=False, variance=np.full((Hh, W), 5.0), **args, **kw)   # out null, the variance alone
            assert none is None and np.array_equal(only_var, var)
            with ft.PinnedArray((Hh, W, 3)) as pinned:
                pinned[:] = 7.0
                hip.temporal_filter(cams[-1], out=pinned, **args, **kw)
                assert np.array_equal(pinned, f64)
            with ft.PinnedArray((Hh, W, 4), dtype=np.uint8) as pinned:
                pinned[:] = 9
                hip.temporal_filter(cams[-1], rgba8=True, out=pinned, **args, **kw)
                assert np.array_equal(pinned, u8)
    # to_frame: ft_fetch_frame returns the result on the tile pixels, the rest of the frame stays, and the next ft_render is the one of a
    # fresh context
    frame0 = hip.fetch_frame(np.zeros((Hh, W, 3)))
    assert np.array_equal(frame0, c)
    f64, _, _ = hip.temporal_filter(cams[-1], to_frame=1, iterations=3, **args)
    frame = hip.fetch_frame(np.zeros((Hh, W, 3)))
    assert np.array_equal(frame[inside], f64[inside]) and np.array_equal(frame[~inside], c[~inside]) and not np.array_equal(frame, c)
    u8, _, _ = hip.temporal_filter(cams[-1], to_frame=1, iterations=3, rgba8=True, **args)       # bytes out, FP64 into the frame
    assert np.array_equal(hip.fetch_frame(np.zeros((Hh, W, 3)))[inside], f64[inside]) and np.array_equal(u8[inside], ft.quantise_rgba8(f64)[inside])
    again, _ = hip.render(cams[-1], W, Hh, 2, jit, seed=2)
    fresh = ft.Context(device=0)
    try:
        scene.lower(fresh)
        want, _ = fresh.render(cams[-1], W, Hh, 2, jit, seed=2)
    finally:
        fresh.close()
    assert np.array_equal(again, want)
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 5. everything else is left alone
@pytest.mark.gpu
def test_everything_else_is_left_alone(hip):
    scene = _load(hip, "sample-soft")
    cam, jit = scene.camera, ft.jitter_pattern(4)
    cams = orbit(cam, 4)
    w, h = W - W % 8, Hh - Hh % 8                                    # an adaptive progressive accumulation needs whole 8x8 blocks
    first, _ = hip.render(cam, w, h, 4, jit, seed=11)
    hip.progressive_begin(cam, w, h, tolerance=0.01, min_samples=2)
    for k in range(3):
        hip.progressive_pass(2, ft.jitter_pattern(2, seed=k + 1), seed=k)
    prog = hip.progressive_fetch()
    # an orbit with a filter call after every accumulate gives bit for bit the history of the orbit without
    states = {}
    for with_filter in (False, True):
        hip.temporal_begin(w, h)
        states[with_filter] = []
        for k, c in enumerate(cams):
            frame, _ = hip.render(c, w, h, 4, jit, seed=k)
            hip.temporal_accumulate(c, 4, jit, sample=1, seed=k, fetch=False)
            if with_filter:
                before, status = hip.temporal_fetch(), hip.temporal_status()
                for demodulate in (1, 0):
                    got, _, _ = hip.temporal_filter(c, 4, jit, sample=1, seed=k, demodulate=demodulate, variance=True)
                    assert not np.array_equal(got, before[0])
                after = hip.temporal_fetch()
                assert all(np.array_equal(x, y) for x, y in zip(before, after)) and hip.temporal_status() == status
                assert np.array_equal(hip.fetch_frame(np.zeros((h, w, 3))), frame)   # without to_frame the frame buffer stays
            states[with_filter].append(hip.temporal_fetch() + (hip.temporal_status(),))
    for x, y in zip(states[False], states[True]):
        assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]
    again, _ = hip.render(cam, w, h, 4, jit, seed=11)
    assert np.array_equal(again, first)
    hip.render(cam, w, h, 4, jit, seed=11, fetch=False)              # ... and once more, straight after a frame of the same signature
    assert np.array_equal(hip.fetch_frame(np.zeros((h, w, 3))), first)
    assert all(np.array_equal(x, y) for x, y in zip(prog, hip.progressive_fetch()))
    hip.progressive_end()
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 6. FT_ERR_STATE
@pytest.mark.gpu
def test_state_errors(hip):
    scene = _load(hip, "hollow-sphere")
    cam, jit = scene.camera, np.zeros((1, 2))
    hip.temporal_end()
    hip._temporal = (W, Hh)                                          # (the Python layer would refuse before the library could)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_filter(cam, 1, jit)
    assert e.value.status == -5 and "ft_temporal_begin" in str(e.value)
    hip.temporal_begin(W, Hh)
    with pytest.raises(ft.FtError) as e:                             # begin, but no accumulate yet
        hip.temporal_filter(cam, 1, jit)
    assert e.value.status == -5 and "ft_temporal_accumulate" in str(e.value)
    hip.render(cam, W, Hh, 1, jit, fetch=False)
    hip.temporal_accumulate(cam, 1, jit, fetch=False)
    hip.temporal_filter(cam, 1, jit, to_frame=1)
    hip.render_rgba8(cam, W, Hh, 1, jit, fetch=False)
    with pytest.raises(ft.FtError) as e:                             # to_frame with an RGBA8 frame in HBM
        hip.temporal_filter(cam, 1, jit, to_frame=1)
    assert e.value.status == -5 and "RGBA8" in str(e.value)
    got, _, _ = hip.temporal_filter(cam, 1, jit)                     # ... which a call without to_frame does not need
    assert np.isfinite(got).all()
    hip.render(cam, W // 2, Hh, 1, jit, fetch=False)
    with pytest.raises(ft.FtError) as e:                             # another size
        hip.temporal_filter(cam, 1, jit, to_frame=1)
    assert e.value.status == -5
    hip.commit()                                                     # a caller's commit ends the accumulation
    hip._temporal = (W, Hh)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_filter(cam, 1, jit)
    assert e.value.status == -5 and "ft_temporal_begin" in str(e.value)
    hip._temporal = None
    two = ft.Context(device=[0, 0])
    try:
        scene.lower(two)
        two._temporal = (W, Hh)
        with pytest.raises(ft.FtError) as e:
            two.temporal_filter(cam, 1, jit)
        assert e.value.status == -4 and "bands" in str(e.value)
    finally:
        two.close()

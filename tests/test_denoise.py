"""ft_denoise (Context.denoise, functracer --denoise N): the FP64 frame in HBM filtered on the device by an edge-avoiding a-trous wavelet
filter guided by ft_render_aov's surfaces.  `reference` below restates the definition of include/functracer_hip.h / DESIGN.md 11 in
numpy; its inputs come from the public API (render, render_aov, progressive_fetch), so it shares no code with k_denoise.

The GPU tests print the figures they assert on; what an MI355X gave is in DESIGN.md 11 "Measured"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import helpers as H

W, Hh = 160, 90
TILES = [(8, 8, 16, 16), (101, 37, 13, 11), (150, 80, 20, 20)]
KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
PARAMS = dict(sigma_colour=0.6, sigma_normal=0.3, sigma_position=1.0, albedo_floor=1e-3, variance_floor=1e-4)


# ---------------------------------------------------------------------------------------------------------------- the definition, in numpy
def _shift(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox] where that lies in the frame, else `fill`."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, ye = max(0, -oy), min(h, h - oy)
    xs, xe = max(0, -ox), min(w, w - ox)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + oy:ye + oy, xs + ox:xe + ox]
    return b


def reference(c, n, p, a, hit, in_tiles, iterations=5, sigma_colour=0.6, sigma_normal=0.3, sigma_position=0.0, demodulate=1, albedo_floor=1e-3,
              use_variance=0, variance_floor=1e-4, se=None):
    """u_N * d for the pixels of `in_tiles` (the others keep c).  c, n, p, a: [h, w, 3]; hit, in_tiles: [h, w] bool."""
    if iterations == 0:
        return c.copy()                                              # bit for bit: no division and multiplication by d
    cls = np.where(in_tiles, hit.astype(np.int8), 2)
    d = np.where((hit & bool(demodulate))[..., None], np.maximum(a, albedo_floor), 1.0)
    with np.errstate(all="ignore"):
        u = c / d
        V = np.ones(c.shape[:2])
        if use_variance:
            r = se / d
            V = variance_floor + (1.0 / 3.0) * (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2])
        for i in range(iterations):
            s = 2 ** i
            num, den = np.zeros_like(u), np.zeros(u.shape[:2])
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq = _shift(cls, s * dy, s * dx, 2)
                    uq = _shift(u, s * dy, s * dx, np.nan)
                    E = np.zeros(u.shape[:2])
                    if sigma_normal > 0:
                        E = E + ((n - _shift(n, s * dy, s * dx, 0.0)) ** 2).sum(-1) / sigma_normal ** 2
                    if sigma_position > 0:
                        E = E + ((p - _shift(p, s * dy, s * dx, 0.0)) ** 2).sum(-1) / sigma_position ** 2
                    if sigma_colour > 0:
                        E = E + ((u - uq) ** 2).sum(-1) / ((sigma_colour * 2.0 ** -i) ** 2 * V)
                    take = (cq == cls) & (cls != 2) & np.isfinite(uq).all(-1) & ~np.isnan(E)
                    wgt = np.where(take, KERNEL[dx + 2] * KERNEL[dy + 2] * np.exp(-E), 0.0)
                    num = num + np.where(take[..., None], wgt[..., None] * uq, 0.0)
                    den = den + wgt
            own = np.isfinite(u).all(-1) & (cls != 2)
            u = np.where(own[..., None], num / den[..., None], u)
        return np.where(in_tiles[..., None], u * d, c)


def _mask(tiles, w=W, h=Hh):
    m = np.zeros((h, w), dtype=bool)
    if tiles is None:
        m[:] = True
    else:
        for (x0, y0, tw, th) in tiles:
            m[max(0, y0):max(0, min(h, y0 + th)), max(0, x0):max(0, min(w, x0 + tw))] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_ft_denoise():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"typedef struct ft_denoise_params\s*\{\s*int32_t iterations, demodulate, use_variance, _pad;\s*"
                     r"double sigma_colour, sigma_normal, sigma_position, albedo_floor, variance_floor;\s*\}\s*ft_denoise_params;", hdr)
    assert re.search(r"int32_t ft_denoise\(ft_context\* ctx, const ft_camera\* cam, int32_t res_h, int32_t res_v, int32_t spp,\s*"
                     r"const double\* jitter_xy, int32_t sample, uint64_t seed, const ft_rect\* tiles, int32_t n_tiles,\s*"
                     r"const ft_denoise_params\* params, int32_t rgba8, void\* out, ft_stats\* stats\);", hdr)
    assert "#define FT_ABI_VERSION 2" in hdr
    assert hasattr(C.CDLL(ft.HIP_LIB), "ft_denoise")
    assert C.sizeof(_capi.ft_denoise_params) == 56


def test_arguments_are_checked_in_order_before_the_device():
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    lib, cam = ft.hip_lib(), ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), H.deg(60), 16 / 9)
    out, jit = np.zeros((18, 32, 3)), np.zeros((4, 2))

    def call(spp=4, sample=0, out=out, null_params=False, **kw):
        p = _capi.ft_denoise_params()
        for k, v in {**_capi.DENOISE_DEFAULTS, **kw}.items():
            setattr(p, k, v)
        return lib.ft_denoise(ctx._ctx, C.byref(cam), 32, 18, spp, _capi.dptr(jit), sample, 1, None, 0, None if null_params else C.byref(p), 0,
                              out.ctypes.data_as(C.c_void_p) if out is not None else None, None)

    assert call(spp=0) == -4                                         # corner sampling: no per-sample geometry ray
    assert call(spp=0, sample=9, iterations=9) == -4                 # ... reported before anything else that is wrong
    assert call(sample=4) == -1 and call(sample=-1) == -1            # sample outside [0, spp)
    assert call(null_params=True) == -1 and call(out=None) == -1
    assert call(iterations=-1) == -1 and call(iterations=7) == -1
    assert call(sigma_colour=-0.1) == -1 and call(sigma_normal=-1.0) == -1 and call(sigma_position=-1e-9) == -1
    assert call(demodulate=1, albedo_floor=0.0) == -1 and call(demodulate=0, albedo_floor=0.0) == -2
    assert call(use_variance=1, variance_floor=0.0) == -1 and call(use_variance=0, variance_floor=-1.0) == -2
    assert call(sample=3, iterations=6) == -2 and call(iterations=0) == -2   # valid, but a host-only context has no device
    with pytest.raises(ValueError):
        ctx.denoise(cam, 32, 18, 1, jit[:1], sigma=1.0)
    ctx.close()


def test_reference_on_hand_worked_cases():
    rng = np.random.default_rng(5)
    on = np.ones((5, 5), dtype=bool)
    z3 = np.zeros((5, 5, 3))
    # a constant frame stays constant: every u_i(q) is the same value, so the weighted mean is that value
    c = np.full((5, 5, 3), 0.375)
    got = reference(c, z3, z3, np.full((5, 5, 3), 0.5), on, on, iterations=3)
    assert np.allclose(got, 0.375, rtol=1e-15, atol=0)
    # zero iterations: c, bit for bit, with and without demodulation
    c = rng.uniform(0, 1, (5, 5, 3))
    assert np.array_equal(reference(c, z3, z3, np.full((5, 5, 3), 0.3), on, on, iterations=0, demodulate=0), c)
    assert np.array_equal(reference(c, z3, z3, np.full((5, 5, 3), 0.3), on, on, iterations=0, demodulate=1), c)
    # two regions with opposite normals, sigma_normal small: |n - n'|^2 / sigma^2 = 4 / 1e-4, exp(-40000) underflows to 0, so each region
    # is filtered on its own and (being constant) keeps its value; without the normal term the edge bleeds
    c = np.zeros((6, 8, 3))
    c[:, :4], c[:, 4:] = 0.2, 0.9
    n = np.zeros((6, 8, 3))
    n[:, :4, 2], n[:, 4:, 2] = 1.0, -1.0
    on = np.ones((6, 8), dtype=bool)
    kept = reference(c, n, np.zeros_like(c), np.ones_like(c), on, on, iterations=2, sigma_colour=0.0, sigma_normal=0.01, demodulate=0)
    assert np.allclose(kept, c, rtol=1e-15, atol=0)
    bled = reference(c, n, np.zeros_like(c), np.ones_like(c), on, on, iterations=2, sigma_colour=0.0, sigma_normal=0.0, demodulate=0)
    assert 0.2 < bled[3, 3, 0] < bled[3, 4, 0] < 0.9
    # classes never mix, pixels outside the tiles neither give nor take, and a NaN pixel stays alone
    c = rng.uniform(0, 1, (6, 8, 3))
    hit = np.zeros((6, 8), dtype=bool)
    hit[:, :3] = True
    tiles = np.ones((6, 8), dtype=bool)
    tiles[:, 6:] = False
    c[2, 1] = np.nan
    got = reference(c, np.zeros_like(c), np.zeros_like(c), np.ones_like(c), hit, tiles, iterations=2, sigma_colour=0.0, demodulate=0)
    assert np.array_equal(got[:, 6:], c[:, 6:]) and np.isnan(got[2, 1]).all() and np.isfinite(np.delete(got.reshape(-1, 3), 2 * 8 + 1, axis=0)).all()
    lo, hi = np.nanmin(c[:, :3]), np.nanmax(c[:, :3])
    assert (np.nan_to_num(got[:, :3], nan=lo) >= lo).all() and (np.nan_to_num(got[:, :3], nan=lo) <= hi).all()
    assert got[:, 3:6].min() >= c[:, 3:6].min() and got[:, 3:6].max() <= c[:, 3:6].max()


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _load(ctx, name, pinhole=False):
    scene = ft.parse_scene_file(H.scene_path(name))
    if pinhole:
        scene.camera.has_focus = 0
    scene.lower(ctx)
    return scene


def _guides(ctx, cam, w, h, spp, jit, sample=0, tiles=None, seed=ft.DEFAULT_SEED):
    g = ctx.render_aov(cam, w, h, spp, jit, sample=sample, seed=seed, tiles=tiles, channels=["n", "p", "colour", "leaf"])
    return g["n"], g["p"], g["colour"], g["leaf"] >= 0


def _check(got, want, mask, what):
    """The two bounds DESIGN.md 3 uses for device against oracle: the contract 1e-4 on every pixel, and 1e-6."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pixels differ"
    nan = np.isnan(want)
    err = H.pixel_errors(np.where(nan, 0.0, got), np.where(nan, 0.0, want))[mask]
    worst = float(err.max()) if err.size else 0.0
    print(f"denoise parity {what}: max rel err {worst:.3e}")
    assert worst < H.PIXEL_RTOL and worst < 1e-6, f"{what}: max rel err {worst:.3e}"
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("name", ["bunny", "hollow-sphere", "moon", "sample-soft"])
def test_device_matches_the_numpy_restatement(hip, name, spp):
    scene = _load(hip, name)
    cam, jit = scene.camera, ft.jitter_pattern(spp)
    sample = spp - 1
    c, _ = hip.render(cam, W, Hh, spp, jit)
    n, p, a, hit = _guides(hip, cam, W, Hh, spp, jit, sample=sample)
    everywhere = _mask(None)
    for iterations in (1, 3, 5):
        for demodulate in (0, 1):
            got, st = hip.denoise(cam, W, Hh, spp, jit, sample=sample, iterations=iterations, demodulate=demodulate, **PARAMS)
            want = reference(c, n, p, a, hit, everywhere, iterations=iterations, demodulate=demodulate, **PARAMS)
            _check(got, want, everywhere, f"{name} x{spp} N={iterations} demodulate={demodulate}")
            assert st["rays_primary"] == W * Hh and st["hits_primary"] == int(hit.sum()) and st["n_launches"] >= iterations + 2
            assert not np.array_equal(got, c)                        # it filtered something


@pytest.mark.gpu
def test_tiles_are_filtered_alone_and_the_rest_is_untouched(hip):
    scene = _load(hip, "hollow-sphere")
    cam, jit = scene.camera, ft.jitter_pattern(2)
    c, _ = hip.render(cam, W, Hh, 2, jit)
    tiles = TILES + [(-5, 60, 30, 12)]                               # one rect clipped by the frame
    inside = _mask(tiles)
    n, p, a, hit = _guides(hip, cam, W, Hh, 2, jit, tiles=tiles)
    out = np.full((Hh, W, 3), 7.0)
    got, _ = hip.denoise(cam, W, Hh, 2, jit, tiles=tiles, out=out, iterations=3, **PARAMS)
    want = reference(c, n, p, a, hit, inside, iterations=3, **PARAMS)
    _check(got, want, inside, "hollow-sphere tiles")
    assert (got[~inside] == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. identity and state
@pytest.mark.gpu
def test_zero_iterations_and_everything_else_left_alone(hip):
    scene = _load(hip, "sample-soft")
    cam, jit = scene.camera, ft.jitter_pattern(4)
    first, _ = hip.render(cam, W, Hh, 4, jit, seed=11)
    before = hip.fetch_frame(np.zeros((Hh, W, 3)))
    same, st = hip.denoise(cam, W, Hh, 4, jit, seed=11, iterations=0)
    assert np.array_equal(same, before) and st["rays_primary"] == 0
    filtered, _ = hip.denoise(cam, W, Hh, 4, jit, seed=11, iterations=4)
    assert not np.array_equal(filtered, before)
    assert np.array_equal(hip.fetch_frame(np.zeros((Hh, W, 3))), before)
    again, _ = hip.render(cam, W, Hh, 4, jit, seed=11)
    assert np.array_equal(again, first)
    # a progressive accumulation is neither read (use_variance = 0) nor changed
    hip.progressive_begin(cam, W - W % 8, Hh - Hh % 8, tolerance=0.01, min_samples=2)
    for k in range(3):
        hip.progressive_pass(2, ft.jitter_pattern(2, seed=k + 1), seed=k)
    mean, se, samples = hip.progressive_fetch()
    hip.denoise(cam, W - W % 8, Hh - Hh % 8, 1, np.zeros((1, 2)), iterations=3)
    mean2, se2, samples2 = hip.progressive_fetch()
    assert np.array_equal(mean, mean2) and np.array_equal(se, se2) and np.array_equal(samples, samples2)
    frame, _ = hip.progressive_pass(2, ft.jitter_pattern(2, seed=9), seed=9)
    hip.progressive_end()
    assert np.isfinite(frame).all()


# ---------------------------------------------------------------------------------------------------------------- 3. RGBA8
@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 3])
def test_rgba8_bytes_are_the_quantised_result(hip, iterations):
    scene = _load(hip, "moon")
    cam, jit = scene.camera, ft.jitter_pattern(2)
    hip.render(cam, W, Hh, 2, jit, fetch=False)
    f64, _ = hip.denoise(cam, W, Hh, 2, jit, iterations=iterations)
    u8, _ = hip.denoise(cam, W, Hh, 2, jit, iterations=iterations, rgba8=True)
    assert np.array_equal(u8, ft.quantise_rgba8(f64))
    with ft.PinnedArray((Hh, W, 4), dtype=np.uint8) as pinned:
        hip.denoise(cam, W, Hh, 2, jit, iterations=iterations, rgba8=True, out=pinned)
        assert np.array_equal(pinned, u8)
    with ft.PinnedArray((Hh, W, 3)) as pinned:
        hip.denoise(cam, W, Hh, 2, jit, iterations=iterations, out=pinned)
        assert np.array_equal(pinned, f64)


# ---------------------------------------------------------------------------------------------------------------- 4. variance path
@pytest.mark.gpu
def test_variance_guided_colour_term(hip):
    scene = _load(hip, "sample-soft")
    cam = scene.camera
    w, h = 160, 88                                                   # adaptive accumulations need tiles of whole 8x8 blocks
    everywhere = _mask(None, w, h)
    params = dict(PARAMS, iterations=4, use_variance=1, variance_floor=1e-4)
    hip.progressive_end()
    hip.render(cam, w, h, 1, np.zeros((1, 2)), fetch=False)
    with pytest.raises(ft.FtError) as e:                             # no accumulation at all
        hip.denoise(cam, w, h, 1, np.zeros((1, 2)), **params)
    assert e.value.status == -5
    hip.progressive_begin(cam, w, h, tolerance=0.0)                  # a plain one keeps no squares
    hip.progressive_pass(2, ft.jitter_pattern(2), seed=1)
    with pytest.raises(ft.FtError) as e:
        hip.denoise(cam, w, h, 1, np.zeros((1, 2)), **params)
    assert e.value.status == -5
    hip.progressive_begin(cam, w, h, tolerance=1e-3, min_samples=2)
    for k in range(3):
        frame, _ = hip.progressive_pass(2, ft.jitter_pattern(2, seed=k + 1), seed=k + 1)
    mean, se, _ = hip.progressive_fetch()
    assert np.array_equal(mean, frame) and se.max() > 0
    jit = ft.jitter_pattern(2, seed=1)
    n, p, a, hit = _guides(hip, cam, w, h, 2, jit, seed=1)
    got, _ = hip.denoise(cam, w, h, 2, jit, seed=1, **params)
    want = reference(mean, n, p, a, hit, everywhere, se=se, **params)
    _check(got, want, everywhere, "sample-soft variance-guided")
    without = reference(mean, n, p, a, hit, everywhere, **dict(params, use_variance=0))
    assert not np.allclose(without, want, rtol=1e-6, atol=0)         # the variance does steer the filter
    with pytest.raises(ft.FtError) as e:                             # other tiles than the accumulation's
        hip.denoise(cam, w, h, 2, jit, seed=1, tiles=[(0, 0, 80, 40)], **params)
    assert e.value.status == -5
    hip.progressive_end()


# ---------------------------------------------------------------------------------------------------------------- 5. it denoises, it keeps edges
@pytest.mark.gpu
def test_soft_light_noise_drops_and_classes_do_not_mix(hip):
    """Conditions, not measurements: the filtered 1-spp frame is closer (RMS) to a 256-spp ft_render of the same request than the raw
    one; a filtered pixel is a convex combination of input pixels of its own class, so it lies within their range - up to the rounding
    of 25 products, a sum and a division, a few ulp: 1e-12 relative is ample; the bunny's miss pixels stay exactly Colour.Zero."""
    scene = _load(hip, "sample-soft", pinhole=True)
    cam = scene.camera
    truth, _ = hip.render(cam, W, Hh, 256, ft.jitter_pattern(256))
    jit = np.zeros((1, 2))
    raw, _ = hip.render(cam, W, Hh, 1, jit)
    got, _ = hip.denoise(cam, W, Hh, 1, jit, iterations=4, sigma_colour=1.0, sigma_normal=0.3, sigma_position=0.0, demodulate=1)
    rms_raw, rms_got = float(np.sqrt(np.mean((raw - truth) ** 2))), float(np.sqrt(np.mean((got - truth) ** 2)))
    print(f"denoise sample-soft 1 spp against 256 spp: RMS raw {rms_raw:.5f}, filtered {rms_got:.5f}, ratio {rms_got / rms_raw:.3f}")
    assert rms_got < rms_raw
    plain, _ = hip.denoise(cam, W, Hh, 1, jit, iterations=4, sigma_colour=1.0, sigma_normal=0.3, sigma_position=0.0, demodulate=0)
    hit = hip.render_aov(cam, W, Hh, 1, jit, channels=["leaf"])["leaf"] >= 0
    for cls in (hit, ~hit):
        if cls.any():
            lo, hi = raw[cls].min(axis=0), raw[cls].max(axis=0)
            slack = 1e-12 * np.maximum(np.abs(lo), np.abs(hi))
            assert (plain[cls] >= lo - slack).all() and (plain[cls] <= hi + slack).all()
    # one sample per pixel, so that the class of a pixel is the class of all its frame holds (with more samples a silhouette pixel
    # whose guide sample misses still carries the colour of the samples that hit)
    bunny = _load(hip, "bunny")
    hip.render(bunny.camera, W, Hh, 1, jit, fetch=False)
    hit = hip.render_aov(bunny.camera, W, Hh, 1, jit, channels=["leaf"])["leaf"] >= 0
    got, _ = hip.denoise(bunny.camera, W, Hh, 1, jit, iterations=5)
    assert hit.any() and (~hit).any() and (got[~hit] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- 6. errors on the device
@pytest.mark.gpu
def test_state_errors_and_non_finite_pixels(hip, golden):
    scene = _load(hip, "hollow-sphere")
    cam, jit = scene.camera, np.zeros((1, 2))
    hip.render_rgba8(cam, W, Hh, 1, jit)
    with pytest.raises(ft.FtError) as e:
        hip.denoise(cam, W, Hh, 1, jit)
    assert e.value.status == -5                                      # the frame in HBM is RGBA8
    hip.render(cam, W, Hh, 1, jit, fetch=False)
    with pytest.raises(ft.FtError) as e:
        hip.denoise(cam, W // 2, Hh, 1, jit)
    assert e.value.status == -5                                      # another size
    fresh = ft.Context(device=0)
    try:
        scene.lower(fresh)
        with pytest.raises(ft.FtError) as e:
            fresh.denoise(cam, W, Hh, 1, jit)
        assert e.value.status == -5                                  # nothing rendered yet
    finally:
        fresh.close()
    two = ft.Context(device=[0, 0])
    try:
        scene.lower(two)
        two.render(cam, W, Hh, 1, jit, fetch=False)
        with pytest.raises(ft.FtError) as e:
            two.denoise(cam, W, Hh, 1, jit)
        assert e.value.status == -4 and "bands" in str(e.value)
    finally:
        two.close()
    # a NaN pixel (negative base under a fractional exponent, Shading.fs:85-87) stays where it is: its neighbours remain finite
    case = [c for c in golden["hand_derived_shading"]["cases"] if c["name"] == "specular_negative_base_fractional_exponent_is_nan"][0]
    H.build_described_scene(hip, case["objects"], case["lights"])
    cam = ft.make_camera((0, 0, -3), (0, 0, 0), (0, 1, 0), H.deg(40.0), 1.0)
    raw, _ = hip.render(cam, 64, 64, 1, jit)
    assert np.isnan(raw).any() and not np.isnan(raw).all()
    for demodulate in (0, 1):
        got, _ = hip.denoise(cam, 64, 64, 1, jit, iterations=5, demodulate=demodulate, **PARAMS)
        assert np.array_equal(np.isnan(got), np.isnan(raw))
        n, p, a, hit = _guides(hip, cam, 64, 64, 1, jit)
        _check(got, reference(raw, n, p, a, hit, _mask(None, 64, 64), iterations=5, demodulate=demodulate, **PARAMS), _mask(None, 64, 64), "NaN frame")


# ---------------------------------------------------------------------------------------------------------------- 7. CLI
@pytest.mark.gpu
def test_cli_denoise_writes_the_python_paths_png(hip, tmp_path):
    scene = _load(hip, "hollow-sphere")
    w, h = scene.resolution
    jit = ft.jitter_pattern(scene.samples)
    hip.render(scene.camera, w, h, scene.samples, jit, fetch=False)
    rgba, _ = hip.denoise(scene.camera, w, h, scene.samples, jit, rgba8=True, iterations=3)
    ft.write_png(tmp_path / "python.png", rgba)
    cli = os.path.join(H.ROOT, "functracer_amd", "lib", "functracer")
    r = subprocess.run([cli, H.scene_path("hollow-sphere"), str(tmp_path / "cli.png"), "--denoise", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Denoised" in r.stderr
    assert (tmp_path / "cli.png").read_bytes() == (tmp_path / "python.png").read_bytes()
    plain = subprocess.run([cli, H.scene_path("hollow-sphere"), str(tmp_path / "plain.png")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and (tmp_path / "plain.png").read_bytes() != (tmp_path / "cli.png").read_bytes()

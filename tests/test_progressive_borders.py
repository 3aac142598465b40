"""Adaptive retirement (ft_progressive_*, tolerance > 0) at its borders and in grouped passes, against the exact twin of
tests/progressive_tools.py: the header's standard error with every operation rounded on its own.  The device's decision persists - a
retired block is never traced again - so every assertion on device results is np.array_equal: the means, the standard errors, the
samples, the retired blocks, the samples traced and the frame a pass returns."""
import ctypes as C
from fractions import Fraction
import math

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import progressive_tools as T

W, H = T.W, T.H
GROUPED = [2, 6, 4, 12, 8, 16, 3, 1]                                # group_log2 1, 1, 2, 2, 3, 4, 0, 0
BORDER_SIZES = [1, 3, 2, 2, 4, 4]                                   # n = 1, 4 (= min_samples), 6, 8, 12, 16
BUILDERS = {"edges": T.build_edges, "lit": T.build_lit, "nan": lambda b: T.build_edges(b, with_nan=True)}

# The frozen example of the finding: a flat block of colour (0.3, 0.7, 0.1) after 5 samples.  Rounded apart, Q / n - m * m is
# 0 or negative in all three channels: se = 0, the block retires under any tolerance.  With the two contractions the device code had
# (Q = fma(c, c, Q), v0 = fma(-m, m, Q / n)) the 0.1 channel keeps v0 = 8.3e-19, se = 4.56e-10: under 1e-12 the block stays.
FROZEN_COLOUR, FROZEN_N, FROZEN_TOLERANCE = (0.3, 0.7, 0.1), 5, 1e-12
FROZEN_CONTRACTED_SE = 4.562530187486071e-10


def _equal(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------- CPU
def _twin_se(S, Q, n):
    return float(T.standard_error(np.full((1, 1, 3), S), np.full((1, 1, 3), Q), np.full((1, 1), n))[0, 0, 0])


def _adversarial_inputs():
    """(S, Q, n) as the accumulation forms them, rounded apart, from samples that are flat, two-valued or random, at magnitudes 1,
    1e-300 and 1e150; and pairs with a Q below its S^2 / n (the clamp) or far above it."""
    rng = np.random.default_rng(20261021)
    out = []
    for scale in (1.0, 1e-300, 1e150, 1e-150):
        for n in (2, 3, 4, 5, 7, 8, 13, 16):
            kinds = [[0.3] * n, [0.7] * n, [0.1] * n, [0.3] * (n // 2) + [0.0] * (n - n // 2), [0.7] + [0.1] * (n - 1),
                     list(rng.random(n)), list(1.0 + 1e-9 * rng.random(n)), list(rng.random(n) ** 8)]
            for samples in kinds:
                S = Q = 0.0
                for c in samples:
                    c = c * scale
                    S = S + c
                    cc = c * c
                    Q = Q + cc
                out.append((S, Q, n))
                out.append((S, Q * (1.0 - 2.0 ** -50), n))          # Q a little under S^2 / n: a negative difference
                out.append((S, Q * 3.0, n))
    return out


def test_twin_against_exact_fractions():
    """The twin's se against the header's formula evaluated exactly (fractions.Fraction) on the same doubles S, Q and n.

    The bound.  With u = 2^-53 the twin forms m = (S/n)(1 + e1), mm = m^2 (1 + e2), q = (Q/n)(1 + e3) and v0 = (q - mm)(1 + e4), all
    |e| <= u, so |v0 - V0| <= u (|Q|/n + 3 (S/n)^2 + |V0|) to first order, V0 the exact difference: the two terms cancel, and the error is
    relative to THEM, not to V0.  delta is that figure with 1 % for the second-order terms, plus (4 + 2 (n - 1)) eta, eta = 5e-324, for
    the operations that may underflow (m * m and Q / n at magnitude 1e-300; the scaling by n / (n - 1) / n, carried back through it).  The
    clamp cannot increase the distance.  se^2 = max(0, v0) / (n - 1) follows by three more operations and a square root, a relative
    (1 + 3u) at the most on se.  With d = delta / (n - 1) and SE the exact value, |sqrt(a) - sqrt(b)| <= min(sqrt |a - b|, |a - b| / sqrt b)
    gives |se - SE| <= min(sqrt d, d / SE) + 4u (SE + sqrt d): checked without a square root as (se - bound)^2 <= SE^2 <= (se + bound)^2,
    with sqrt d and SE taken from above in doubles (a factor 1 + 2^-50).

    Where every intermediate result is exactly representable nothing rounds and the agreement is bitwise: two samples a, b of few bits
    give se = |a - b| / 2 through exact steps."""
    worst = 0.0
    for S, Q, n in _adversarial_inputs():
        se = _twin_se(S, Q, n)
        se2, d = T.se_error_bound(S, Q, n)
        up = 1.0 + 2.0 ** -50
        root_d, SE = math.sqrt(float(d)) * up + 1e-320, math.sqrt(float(se2)) * up
        first = min(root_d, float(d) / SE * up) if SE > 0.0 else root_d
        bound = Fraction(first) + 4 * Fraction(T.U) * (Fraction(SE) + Fraction(root_d))
        lo, hi = max(Fraction(0), Fraction(se) - bound), Fraction(se) + bound
        assert lo * lo <= se2 <= hi * hi, f"S {S!r} Q {Q!r} n {n}: se {se!r} against exact se^2 {float(se2)!r}, bound {float(bound)!r}"
        if se2 > 0:
            worst = max(worst, abs(se - math.sqrt(float(se2))) / float(bound))
    assert worst > 1e-3, "the bound is far from what the cases reach: they exercise nothing"
    exact = 0
    for a in (0.5, 0.75, 1.25, 3.0, 2.0 ** -20, 1.0 + 2.0 ** -20):
        for b in (0.25, 1.0, 0.0, 2.0 ** -10):
            S, Q = a + b, a * a + b * b
            assert Fraction(S) == Fraction(a) + Fraction(b) and Fraction(Q) == Fraction(a) ** 2 + Fraction(b) ** 2   # nothing rounded
            assert _twin_se(S, Q, 2) == abs(a - b) / 2.0 and T.exact_se_squared(S, Q, 2)[0] == Fraction(abs(a - b) / 2.0) ** 2
            exact += 1
    assert exact == 24


def test_the_clamp_fires_on_flat_pixels():
    """A pixel whose samples are all one non-dyadic colour has Q / n - m * m < 0 for some n: the clamp is what makes its se 0."""
    fired = []
    for c in (0.1, 0.3, 0.7):
        for n in range(2, 17):
            se, v0 = T.se_rounded_apart([c] * n)
            if v0 < 0.0:
                fired.append((c, n))
                assert se == 0.0 and _twin_se(*_sums([c] * n), n) == 0.0
    assert len(fired) >= 3 and {c for c, _ in fired} == {0.1, 0.3, 0.7}, fired


def _sums(samples):
    S = Q = 0.0
    for c in samples:
        S = S + c
        cc = c * c
        Q = Q + cc
    return S, Q


def test_contracted_arithmetic_changes_a_verdict():
    """The frozen example: the twin retires the flat block, the arithmetic the device code had before it followed the header does not -
    and the other way round at n = 3 - so a device that contracts cannot pass the GPU tests below."""
    apart = [T.se_rounded_apart([c] * FROZEN_N)[0] for c in FROZEN_COLOUR]
    fused = [T.se_contracted([c] * FROZEN_N)[0] for c in FROZEN_COLOUR]
    assert apart == [0.0, 0.0, 0.0] and fused == [0.0, 0.0, FROZEN_CONTRACTED_SE]
    assert FROZEN_TOLERANCE < 1e-9 and max(apart) <= FROZEN_TOLERANCE < max(fused)
    frames = [np.broadcast_to(np.array(FROZEN_COLOUR), (8, 8, 3)).copy() for _ in range(FROZEN_N)]
    run = T.accumulate(frames, [2, 3], FROZEN_TOLERANCE, FROZEN_N)
    assert not run[0]["retired"].any() and run[1]["retired"].all() and (run[1]["se"] == 0.0).all()
    # the reverse: at n = 3 the twin reports 2.6e-9 and 9.1e-9 where the contracted 0.3 channel is 0
    assert T.se_rounded_apart([0.3] * 3)[0] == 2.634178031930877e-09 and T.se_contracted([0.3] * 3)[0] == 0.0
    # and in general the two differ in bits on about half of all pixels (random samples, n = 2 .. 16)
    rng = np.random.default_rng(7)
    differ = sum(T.se_rounded_apart(s)[0] != T.se_contracted(s)[0] for s in (list(rng.random(int(rng.integers(2, 17)))) for _ in range(300)))
    assert differ > 60, differ


def test_edges_scene_reaches_its_cases_on_the_oracle():
    """Indicative only (the GPU half asserts the same on the device's own frames): with the oracle's frames the scene has flat, background
    and two-valued blocks and the border search finds its picks."""
    orc = O.Oracle()
    cam = T.build_edges(orc)
    jit = ft.jitter_pattern(sum(BORDER_SIZES))
    frames = T.single_sample_frames(orc, cam, jit, seed=None)
    kinds = T.block_kinds(frames)
    assert kinds["flat"].sum() >= 2 and kinds["background"].sum() >= 4 and kinds["two_valued"].sum() >= 4
    for colour in T.COLOURS:
        assert any((f.reshape(-1, 3) == np.array(colour)).all(axis=1).any() for f in frames), f"no pixel shows {colour} as it is"
    free, picks = T.border_picks(frames, BORDER_SIZES, 4)
    chosen = T.choose_picks(picks, free, BORDER_SIZES, 4, kinds["two_valued"])
    assert len({p[2] for p in chosen}) >= 4


def test_host_only_context_refuses_the_accumulations_used_here():
    ctx = ft.Context(host_only=True)
    cam = T.build_edges(ctx)
    for w, h in ((64, 32), (64, 48)):
        for tolerance in (math.inf, 5e-324, 1e-12):
            for min_samples in (2, 5):
                assert ctx._lib.ft_progressive_begin(ctx._ctx, C.byref(cam), w, h, 8, None, 0, tolerance, min_samples) == -2
    ctx.close()


def test_planner_and_grouping_twins():
    assert [T.group_log2(s) for s in GROUPED] == [1, 1, 2, 2, 3, 4, 0, 0]
    assert [T.group_log2(s, 4) for s in GROUPED] == [1, 1, 2, 2, 2, 2, 0, 0] and [T.group_log2(s, 1) for s in GROUPED] == [0] * 8
    assert T.plan_windows(2048, 3, 512, True) == [704, 704, 640] and T.plan_windows(2048, 3, 512, False) == [320] * 6 + [128]
    assert T.plan_windows(2048, 16, 16 << 20, True) == [2048]


# ------------------------------------------------------------------------------------------------------------------------- GPU
_cache = {}


def _scene(hip, name, n_frames=sum(GROUPED)):
    """Commits scene `name` on the session's context and returns (camera, jitter pattern, the device's single-sample frames, the blocks
    k_classify finishes: those a one-block ft_render reports as culled).  Rendered once per scene."""
    cam = BUILDERS[name](hip)
    if name not in _cache:
        jit = ft.jitter_pattern(n_frames)
        frames = T.single_sample_frames(hip, cam, jit)
        finished = np.zeros((H // 8, W // 8), dtype=bool)
        for by in range(H // 8):
            for bx in range(W // 8):
                _, st = hip.render(cam, W, H, 1, jit[:1], seed=7, tiles=[(8 * bx, 8 * by, 8, 8)], fetch=False)
                assert st["rays_primary_culled"] in (0, 64)
                finished[by, bx] = st["rays_primary_culled"] == 64
        _cache[name] = (jit, frames, finished)
    return (cam,) + _cache[name]


def _accumulate_on_device(ctx, cam, jit, sizes, tolerance, min_samples, tiles=None, rgba8=False, prefill=None):
    """The passes on the device: per pass the frame returned, the pass's stats, the status and the fetched state."""
    ctx.progressive_begin(cam, W, H, tiles=tiles, tolerance=tolerance, min_samples=min_samples)
    out, at = [], 0
    for spp in sizes:
        buf = None if prefill is None else np.full((H, W, 3), prefill)
        frame, st = ctx.progressive_pass(spp, jit[at:at + spp], seed=7, rgba8=rgba8, out=buf)
        at += spp
        mean, se, samples = ctx.progressive_fetch()
        out.append({"frame": frame, "stats": st, "status": ctx.progressive_status(), "mean": mean, "se": se, "samples": samples})
    ctx.progressive_end()
    return out


def _assert_equals_twin(got, twin, what, frame_is_mean=True):
    for k, (g, t) in enumerate(zip(got, twin)):
        where = f"{what}, pass {k}"
        assert _equal(g["samples"], t["n"]), f"{where}: samples per pixel"
        assert _equal(g["mean"], t["mean"]), f"{where}: mean"
        if frame_is_mean:
            assert _equal(g["frame"], t["mean"]), f"{where}: the frame the pass returned"
        differ = int((~((g["se"] == t["se"]) | ((g["se"] != g["se"]) & (t["se"] != t["se"])))).sum())
        assert _equal(g["se"], t["se"]), f"{where}: standard errors differ in {differ} of {t['se'].size} values"
        st = g["status"]
        assert st["blocks_retired"] == int(t["retired"].sum()), f"{where}: {st['blocks_retired']} blocks retired, the twin retires {int(t['retired'].sum())}"
        assert st["samples_traced"] == t["traced"], f"{where}: {st['samples_traced']} samples traced, the twin's live blocks have {t['traced']}"
        assert st["passes"] == k + 1 and st["min_samples"] == t["n"][t["n"] > 0].min() and st["max_samples"] == t["n"].max(), where


def _retired_pixels(samples, total):
    """What the fetched state tells about retirement: a pixel with fewer samples than the passes offered sits in a retired block."""
    return samples < total


@pytest.mark.gpu
@pytest.mark.parametrize("wave_samples", [0, 1, 2, 4, 16])
@pytest.mark.parametrize("name", ["edges", "lit"])
def test_grouped_passes_with_squares(hip, name, wave_samples):
    """Passes of 2 .. 16 samples take resolve_grouped<1 .. 4, SQ = true> (and, under option wave_samples, narrower groups or the plain
    loop for the same samples): S, Q and every verdict are the twin's whatever the grouping."""
    cam, jit, frames, finished = _scene(hip, name)
    tol, twin = T.pick_tolerance(frames, GROUPED, 4)
    twin = T.accumulate(frames, GROUPED, tol, 4, finished=finished)
    counts = [int(t["retired"].sum()) for t in twin]
    assert 0 < counts[-1] < 32 and len(set(counts)) >= 3, counts
    try:
        hip.set_option("wave_samples", wave_samples)
        got = _accumulate_on_device(hip, cam, jit, GROUPED, tol, 4)
    finally:
        hip.set_option("wave_samples", 0)
    _assert_equals_twin(got, twin, f"{name}, wave_samples {wave_samples}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "lit"])
def test_borders_of_the_rule(hip, name):
    """se == tolerance retires (the rule is <=), one step less does not: for picks (block, pass k*, T = the block's largest se there, a
    strict new minimum over its deciding passes) the accumulation runs under T, one and two steps below and above, and equals the twin
    every time - the picked block decides at the border, every other block is a control."""
    cam, jit, frames, finished = _scene(hip, name)
    frames, jit = frames[:sum(BORDER_SIZES)], jit[:sum(BORDER_SIZES)]
    kinds = T.block_kinds(frames)
    free, picks = T.border_picks(frames, BORDER_SIZES, 4)
    chosen = T.choose_picks(picks, free, BORDER_SIZES, 4, kinds["two_valued"] if name == "edges" else None)
    assert len({p[2] for p in chosen}) >= 4 and any(p[2] == 1 for p in chosen) and any(p[2] == len(BORDER_SIZES) - 1 for p in chosen)
    for by, bx, k_star, tol_at in chosen:
        for tol in T.five_tolerances(tol_at):
            twin = T.accumulate(frames, BORDER_SIZES, tol, 4, finished=finished)
            retires_at = [k for k, t in enumerate(twin) if t["retired"][by, bx]]
            if tol >= tol_at:
                assert retires_at and retires_at[0] == k_star, f"block ({by}, {bx}) under {tol!r}: the twin retires it after passes {retires_at}"
            else:
                assert not retires_at or retires_at[0] > k_star, f"block ({by}, {bx}) under {tol!r}: retired one step below its border"
            got = _accumulate_on_device(hip, cam, jit, BORDER_SIZES, tol, 4)
            _assert_equals_twin(got, twin, f"{name}, block ({by}, {bx}), pass {k_star}, tolerance {tol!r} (border {tol_at!r})")


@pytest.mark.gpu
@pytest.mark.parametrize("min_samples", [2, 5])
@pytest.mark.parametrize("tolerance", [5e-324, 1e-300, 1e-12, math.inf])
def test_flat_blocks_and_tiny_tolerances(hip, tolerance, min_samples):
    """On the unlit squares a flat block's se is 0 or some 1e-9 of its colour, by the rounding of Q / n - m * m alone: the retired set is
    the twin's at every pass, and - from the fetched values alone - every retired block's se is <= tolerance and every live deciding
    block has one that is not: the header's sentence."""
    cam, jit, frames, finished = _scene(hip, "edges")
    sizes = [1, 1, 1, 2, 3, 4, 4]                                   # n = 1, 2, 3, 5, 8, 12, 16
    twin = T.accumulate(frames, sizes, tolerance, min_samples, finished=finished)
    got = _accumulate_on_device(hip, cam, jit, sizes, tolerance, min_samples)
    _assert_equals_twin(got, twin, f"tolerance {tolerance!r}, min_samples {min_samples}")
    flat = T.block_kinds(frames[:16])["flat"]
    assert flat.sum() >= 2 and (twin[-1]["retired"][flat].all() or tolerance < 1e-9)
    total = 0
    for k, g in enumerate(got):
        total += sizes[k]
        gone_before = _retired_pixels(g["samples"], total)          # retired in an earlier pass
        values = T.per_block(g["se"])
        within = np.all(values <= tolerance, axis=2)
        n_block = g["samples"][::8, ::8]
        retired_now = twin[k]["retired"]
        assert (within[retired_now]).all(), f"pass {k}: a retired block reports a standard error above the tolerance"
        assert gone_before[::8, ::8][~retired_now].sum() == 0
        live_deciding = ~retired_now & (n_block >= min_samples)
        assert not within[live_deciding].any(), f"pass {k}: a live block with min_samples has every standard error within the tolerance"
        assert int(retired_now.sum()) == g["status"]["blocks_retired"]


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,min_samples,first_judged", [([1, 1, 1, 1], 2, 1), ([4, 4], 5, 1), ([3, 2], 5, 1)])
def test_min_samples_edges(hip, sizes, min_samples, first_judged):
    """tolerance = inf: a block without a NaN retires at the first pass that ends with n >= min_samples and not before - after one sample
    (n - 1 = 0: 0 * inf on the device, se reported 0) nothing has retired; n == min_samples exactly ([3, 2]) and a pass that carries n across
    it ([4, 4]) both judge."""
    cam, jit, frames, finished = _scene(hip, "nan")
    twin = T.accumulate(frames, sizes, math.inf, min_samples, finished=finished)
    got = _accumulate_on_device(hip, cam, jit, sizes, math.inf, min_samples)
    _assert_equals_twin(got, twin, f"sizes {sizes}, min_samples {min_samples}")
    for k in range(first_judged):
        assert got[k]["status"]["blocks_retired"] == 0, f"pass {k}: retired below min_samples"
    if sizes[0] == 1:
        assert (got[0]["se"] == 0.0).all()
    nan_block = T.per_block(np.isnan(twin[first_judged]["S"])).any(axis=2)
    assert 0 < nan_block.sum() < 8
    assert got[first_judged]["status"]["blocks_retired"] == 32 - int(nan_block.sum())
    assert (got[first_judged]["samples"][::8, ::8][~nan_block] == sum(sizes[:first_judged + 1])).all()


@pytest.mark.gpu
def test_finished_and_retired_blocks_beside_active_ones(hip):
    """k_classify finishes the background blocks of the bounded scene: resolve's untraced path, with squares, gives them the pass's samples
    (block_pos == -1) and judges them - they retire at min_samples with se = 0 - and copies retired blocks through.  All blocks share one n
    until they retire and a finished block's se is 0, so a finished block never outlives the first deciding pass: active and finished
    blocks meet in the passes up to it, active and retired ones afterwards, never all three."""
    cam, jit, frames, finished = _scene(hip, "edges")
    sizes, min_samples = [1, 2, 1, 2, 2, 4], 4
    tol, _ = T.pick_tolerance(frames, sizes, min_samples)
    twin = T.accumulate(frames, sizes, tol, min_samples, finished=finished)
    got = _accumulate_on_device(hip, cam, jit, sizes, tol, min_samples)
    _assert_equals_twin(got, twin, "three states")
    assert 4 <= finished.sum() < 32 and (T.per_block(np.stack(frames[:12]).max(axis=(0, 3))[..., None])[finished] == 0.0).all()
    for k in range(3):                                              # up to the first deciding pass: active and finished blocks
        live = int(twin[k]["live"].sum())
        assert live == 32 - finished.sum() and got[k]["status"]["samples_traced"] == live * 64 * sizes[k]
        assert (got[k]["samples"] == sum(sizes[:k + 1])).all(), f"pass {k}: a finished block did not gain the pass's samples"
    assert twin[1]["retired"].sum() == 0 and twin[2]["retired"][finished].all() and (twin[2]["block_se"][finished] == 0.0).all()
    assert (got[2]["se"][T.per_pixel(finished)] == 0.0).all() and (got[2]["samples"][T.per_pixel(finished)] == min_samples).all()
    for k in range(3, len(sizes)):                                  # afterwards: active and retired blocks
        gone = twin[k - 1]["retired"]
        assert 0 < twin[k]["live"].sum() == 32 - gone.sum() < 32 - finished.sum()
        px = T.per_pixel(gone)
        for key in ("mean", "se", "samples", "frame"):
            assert _equal(got[k][key][px], got[k - 1][key][px]), f"pass {k}: {key} of a retired block changed"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "lit"])
def test_passes_cut_into_windows(hip, name):
    """chunk_samples 512 cuts the passes into up to 32 windows of whole blocks (the planner's rule, checked against ft_stats.n_chunks), some
    with a short last window: the accumulation equals the single-window one and the twin."""
    cam, jit, frames, finished = _scene(hip, name)
    tol, _ = T.pick_tolerance(frames, GROUPED, 4)
    twin = T.accumulate(frames, GROUPED, tol, 4, finished=finished)
    whole = _accumulate_on_device(hip, cam, jit, GROUPED, tol, 4)
    try:
        hip.set_option("chunk_samples", 512)
        cut = _accumulate_on_device(hip, cam, jit, GROUPED, tol, 4)
    finally:
        hip.set_option("chunk_samples", 16 << 20)
    plans = [T.plan_windows(W * H, spp, 512, name == "edges") for spp in GROUPED]
    assert [g["stats"]["n_chunks"] for g in cut] == [len(p) for p in plans] and all(g["stats"]["n_chunks"] == 1 for g in whole)
    assert max(len(p) for p in plans) >= 3 and any(len(p) >= 3 and p[-1] < p[0] for p in plans), plans
    _assert_equals_twin(cut, twin, f"{name}, windows")
    for k, (a, b) in enumerate(zip(cut, whole)):
        for key in ("frame", "mean", "se", "samples"):
            assert _equal(a[key], b[key]), f"pass {k}: {key} differs from the single-window pass"
        assert a["status"] == b["status"]


@pytest.mark.gpu
def test_adaptive_accumulation_over_tiles(hip):
    """Two tiles of whole blocks: the twin restricted to them; outside, the mean, se and samples are 0 and `out` keeps what it held."""
    cam, jit, frames, finished = _scene(hip, "edges")
    tiles, sizes = [(8, 8, 16, 8), (40, 0, 24, 16)], [2, 2, 4, 3, 5]
    inside = T.tile_blocks(tiles, W, H)
    tol, _ = T.pick_tolerance(frames, sizes, 4, inside=inside)
    twin = T.accumulate(frames, sizes, tol, 4, finished=finished, inside=inside)
    got = _accumulate_on_device(hip, cam, jit, sizes, tol, 4, tiles=tiles, prefill=-1.0)
    _assert_equals_twin(got, twin, "tiles", frame_is_mean=False)
    px = T.per_pixel(inside)
    assert inside.sum() == 8 and 0 < twin[-1]["retired"].sum() < 8
    for k, g in enumerate(got):
        assert g["status"]["blocks"] == 8
        assert _equal(g["frame"][px], twin[k]["mean"][px]) and (g["frame"][~px] == -1.0).all(), f"pass {k}: the frame"
        assert (g["mean"][~px] == 0.0).all() and (g["se"][~px] == 0.0).all() and (g["samples"][~px] == 0).all()
        assert not twin[k]["retired"][~inside].any()


@pytest.mark.gpu
def test_rgba8_frames_of_adaptive_passes(hip):
    """Block by block the bytes of ft_render_rgba8 over that block's own prefix of the pattern."""
    cam, jit, frames, finished = _scene(hip, "edges")
    sizes = [2, 2, 4, 8]
    tol, _ = T.pick_tolerance(frames, sizes, 4)
    twin = T.accumulate(frames, sizes, tol, 4, finished=finished)
    assert len(np.unique(twin[-1]["n"])) >= 2
    got = _accumulate_on_device(hip, cam, jit, sizes, tol, 4, rgba8=True)
    _assert_equals_twin(got, twin, "RGBA8", frame_is_mean=False)
    want = {}
    for k, g in enumerate(got):
        assert g["frame"].dtype == np.uint8 and g["frame"].shape == (H, W, 4)
        for n in np.unique(twin[k]["n"]):
            if int(n) not in want:
                want[int(n)] = hip.render_rgba8(cam, W, H, int(n), jit[:n], seed=7)[0]
            sel = twin[k]["n"] == n
            assert np.array_equal(g["frame"][sel], want[int(n)][sel]), f"pass {k}: blocks of {n} samples"


@pytest.mark.gpu
def test_a_nan_never_retires(hip):
    """tolerance = inf retires everything that can retire at min_samples; a block that holds a NaN pixel (a specular exponent of NaN)
    stays live, is traced in every pass, and reports NaN means and standard errors there."""
    cam, jit, frames, finished = _scene(hip, "nan")
    sizes, min_samples = [1, 1, 2, 4, 3], 2
    twin = T.accumulate(frames, sizes, math.inf, min_samples, finished=finished)
    got = _accumulate_on_device(hip, cam, jit, sizes, math.inf, min_samples)
    _assert_equals_twin(got, twin, "NaN")
    nan_px = np.isnan(twin[1]["S"]).any(axis=2)                     # after min_samples samples
    nan_block = T.per_block(nan_px[..., None]).any(axis=2)
    assert nan_px.sum() >= 4 and 0 < nan_block.sum() < 8 and not finished[nan_block].any()
    total = 0
    for k, g in enumerate(got):
        total += sizes[k]
        assert (g["samples"][T.per_pixel(nan_block)] == total).all(), f"pass {k}: a NaN block stopped gaining samples"
        if k >= 1:
            assert np.isnan(g["mean"][nan_px]).any(axis=1).all()
            assert np.isnan(g["se"][nan_px]).any(axis=1).all()
            assert g["status"]["blocks_retired"] == 32 - nan_block.sum()
            assert (g["samples"][T.per_pixel(~nan_block)] == min_samples).all()
        if k >= 2:
            assert g["status"]["samples_traced"] == int(nan_block.sum()) * 64 * sizes[k]


@pytest.mark.gpu
def test_multi_device_grouped_passes(hip):
    """Every device accumulates and retires its 8-row bands in grouped passes, on the classified scene and on the mask-only one: frames,
    fetch and status are the single device's and the twin's."""
    import torch
    n_dev = torch.cuda.device_count()
    ordinals = list(range(min(n_dev, 4))) if n_dev > 1 else [0, 0, 0]
    sizes = [2, 4, 6, 4]
    multi = ft.Context(device=ordinals)
    try:
        for name in ("edges", "lit"):
            cam, jit, frames, finished = _scene(hip, name)
            tol, _ = T.pick_tolerance(frames, sizes, 4)
            twin = T.accumulate(frames, sizes, tol, 4, finished=finished)
            assert 0 < twin[-1]["retired"].sum() < 32
            single = _accumulate_on_device(hip, cam, jit, sizes, tol, 4)
            BUILDERS[name](multi)
            shared = _accumulate_on_device(multi, cam, jit, sizes, tol, 4)
            _assert_equals_twin(single, twin, f"{name}, one device")
            _assert_equals_twin(shared, twin, f"{name}, devices {ordinals}")
            for k, (a, b) in enumerate(zip(shared, single)):
                assert a["status"] == b["status"] and all(_equal(a[key], b[key]) for key in ("frame", "mean", "se", "samples")), f"{name}, pass {k}"
    finally:
        multi.close()

"""An exact twin of adaptive progressive accumulation (ft_progressive_*, include/functracer_hip.h) in plain numpy, and exact models of
its arithmetic for the CPU half of tests/test_progressive_borders.py.

The twin is the expectation: the header's formula, var = max(0, Q/n - (S/n)^2) * n / (n - 1), se = sqrt(var / n), with EVERY operation
rounded on its own - one IEEE double operation per numpy ufunc call, nothing fused - and Q the running sum of the samples' squares, each
square rounded before it is added.  That is how the host (ft_progressive_fetch, built with -ffp-contract=off) and k_denoise_scatter
evaluate it, and how the device has to judge a block: a block that retires is never traced again, so the decision must not hang on
whether a compiler contracted a multiply into an add."""
from fractions import Fraction
import math

import numpy as np

import functracer_amd as ft

U = 2.0 ** -53                                                      # unit roundoff of a double
ETA = 5e-324                                                        # the smallest subnormal: what one underflowing operation can lose


# ------------------------------------------------------------------------------------------------------------------ the twin
def standard_error(S, Q, n):
    """se per pixel and channel from S, Q [h, w, 3] and n [h, w] (integers), one rounding per line; 0 where n < 2 (as ft_progressive_fetch
    reports it).  A NaN stays a NaN through the clamp (NaN < 0 is false), as on the device."""
    dn = np.asarray(n).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        m = np.divide(S, dn)
        mm = np.multiply(m, m)
        q = np.divide(Q, dn)
        v0 = np.subtract(q, mm)
        c = np.where(v0 < 0.0, 0.0, v0)
        a = np.multiply(c, dn)
        n1 = np.subtract(dn, 1.0)                                   # exact
        b = np.divide(a, n1)
        d = np.divide(b, dn)
        se = np.sqrt(d)
    return np.where((np.asarray(n) >= 2)[..., None], se, 0.0)


def mean_of(S, n):
    """S / n, 0 where a pixel has no sample (ft_progressive_fetch)."""
    dn = np.asarray(n).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        m = np.divide(S, dn)
    return np.where((np.asarray(n) > 0)[..., None], m, 0.0)


def per_block(x):
    """[h, w, ...] -> [h / 8, w / 8, 64 * ...]: the values of every 8x8 block."""
    h, w = x.shape[:2]
    return np.moveaxis(x.reshape(h // 8, 8, w // 8, 8, -1), 1, 2).reshape(h // 8, w // 8, -1)


def per_pixel(b):
    """A per-block array [h / 8, w / 8] as a per-pixel one."""
    return np.repeat(np.repeat(b, 8, 0), 8, 1)


def tile_blocks(tiles, w, h):
    """The blocks [h / 8, w / 8] an accumulation over `tiles` (x0, y0, w, h; all multiples of 8, so that the blocks of the pixel list
    are the frame's) holds; every block when tiles is None."""
    inside = np.zeros((h // 8, w // 8), dtype=bool)
    if tiles is None:
        inside[:] = True
        return inside
    for x0, y0, tw, th in tiles:
        assert x0 % 8 == 0 and y0 % 8 == 0 and tw % 8 == 0 and th % 8 == 0
        inside[y0 // 8:(y0 + th) // 8, x0 // 8:(x0 + tw) // 8] = True
    return inside


def accumulate(frames, sizes, tolerance, min_samples, finished=None, inside=None):
    """Adaptive accumulation of the single-sample frames c_k [h, w, 3] in passes of `sizes` samples.  tolerance None: nothing retires
    (the free run).  finished: per pass (or one for all) the blocks [h / 8, w / 8] the device finishes without tracing them - they gain
    the pass's samples to n with S and Q unchanged, which is what adding their zero samples gives, so the mask only changes `live`.
    inside: the blocks of the accumulation (tile_blocks).  One dict per pass: S, Q, n, se, mean, retired (after the pass), live (the blocks
    the pass traced), traced (their samples), block_se (each block's largest se; NaN if it holds one)."""
    h, w = frames[0].shape[:2]
    assert h % 8 == 0 and w % 8 == 0 and sum(sizes) <= len(frames)
    inside = np.ones((h // 8, w // 8), dtype=bool) if inside is None else inside
    S, Q, n = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.int64)
    retired = np.zeros((h // 8, w // 8), dtype=bool)
    out, at = [], 0
    for k, spp in enumerate(sizes):
        gets = inside & ~retired                                    # blocks that receive the pass's samples
        fin = np.zeros_like(gets) if finished is None else (finished[k] if isinstance(finished, (list, tuple)) else finished)
        live = gets & ~fin
        px = per_pixel(gets)
        for c in frames[at:at + spp]:
            with np.errstate(all="ignore"):
                s1 = np.add(S, c)
                cc = np.multiply(c, c)                              # rounded on its own ...
                q1 = np.add(Q, cc)                                  # ... then added
            S = np.where(px[..., None], s1, S)
            Q = np.where(px[..., None], q1, Q)
        at += spp
        n = np.where(px, n + spp, n)
        se = standard_error(S, Q, n)
        values = per_block(se)
        with np.errstate(all="ignore"):
            block_se = values.max(axis=2)                           # (np.max hands a NaN on)
            within = np.all(values <= tolerance, axis=2) if tolerance is not None else np.zeros_like(gets)   # a NaN satisfies nothing
        deciding = gets & (n[::8, ::8] >= min_samples)
        retired = retired | (deciding & within)
        out.append({"S": S, "Q": Q, "n": n, "se": se, "mean": mean_of(S, n), "retired": retired.copy(), "live": live, "deciding": deciding,
                    "traced": int(live.sum()) * 64 * spp, "block_se": block_se})
    return out


def pick_tolerance(frames, sizes, min_samples, inside=None):
    """A tolerance taken from the free run - the largest se of some block at some deciding pass - under which blocks retire at two
    different passes at least and some block stays live to the end.  No margin: the tests hold the device to the twin exactly."""
    free = accumulate(frames, sizes, None, min_samples, inside=inside)
    n_blocks = free[0]["retired"].size if inside is None else int(inside.sum())
    values = np.unique(np.concatenate([p["block_se"][p["deciding"]] for p in free]))
    values = values[np.isfinite(values) & (values > 0)]
    best = None
    for q in (0.5, 0.4, 0.6, 0.3, 0.7, 0.2, 0.8, 0.1, 0.9):
        tol = float(values[int(q * (values.size - 1))])
        run = accumulate(frames, sizes, tol, min_samples, inside=inside)
        counts = [int(p["retired"].sum()) for p in run]
        steps = sum(1 for a, b in zip([0] + counts, counts) if b > a)
        if 0 < counts[-1] < n_blocks and steps >= 2:
            return tol, run
        if best is None and 0 < counts[-1] < n_blocks:
            best = (tol, run)
    assert best is not None, "no tolerance of the free run retires some blocks and not all"
    return best


def border_picks(frames, sizes, min_samples):
    """(block row, block column, pass k*, T) for every block and deciding pass at which the block's largest se, T > 0, is a strict new
    minimum over its deciding passes: under tolerance T the block retires exactly after pass k*, under nextafter(T, 0) it does not."""
    free = accumulate(frames, sizes, None, min_samples)
    bh, bw = free[0]["block_se"].shape
    picks = []
    for by in range(bh):
        for bx in range(bw):
            low = math.inf
            for k, p in enumerate(free):
                if not p["deciding"][by, bx]:
                    continue
                v = float(p["block_se"][by, bx])
                if not v == v:                                      # a NaN block is never a pick (and never retires)
                    break
                if v < low:
                    if v > 1e-300:
                        picks.append((by, bx, k, v))
                    low = v
    return free, picks


def choose_picks(picks, free, sizes, min_samples, want_block=None):
    """At least four picks with distinct k*: one at the pass where n == min_samples, one at the last pass, one (want_block: a mask of
    blocks) on a wanted kind of block; the rest from other passes.  Raises AssertionError where the scene does not offer them."""
    n_after = np.cumsum(sizes)
    chosen = {}

    def take(cond, what):
        used = {(p[0], p[1]) for p in chosen.values()}
        for fresh_block in (True, False):                           # another block than the picks so far, where there is one
            for p in picks:
                if p[2] not in chosen and cond(p) and (not fresh_block or (p[0], p[1]) not in used):
                    chosen[p[2]] = p
                    return
        raise AssertionError(f"the border search found no pick {what}")

    at_min = [k for k in range(len(sizes)) if n_after[k] == min_samples]
    assert at_min, "no pass ends at n == min_samples"
    if want_block is not None:                                      # first, so that no other choice takes its pass
        take(lambda p: want_block[p[0], p[1]] and p[2] not in (at_min[0], len(sizes) - 1), "on a block of the wanted kind")
    take(lambda p: p[2] == at_min[0], "at n == min_samples")
    take(lambda p: p[2] == len(sizes) - 1, "at the last pass")
    for k in range(len(sizes)):
        if len(chosen) >= 4:
            break
        if k not in chosen and any(p[2] == k for p in picks):
            take(lambda p, k=k: p[2] == k, f"at pass {k}")
    assert len(chosen) >= 4, f"the border search found picks at {len(chosen)} distinct passes only"
    return [chosen[k] for k in sorted(chosen)]


def five_tolerances(T):
    """T, one and two steps below, one and two steps above."""
    down1, up1 = np.nextafter(T, 0.0), np.nextafter(T, np.inf)
    return [float(np.nextafter(down1, 0.0)), float(down1), float(T), float(up1), float(np.nextafter(up1, np.inf))]


def plan_windows(n_pix, spp, chunk_samples, host_classified):
    """The windows plan_chunks (ft_frame.cpp) cuts a pass's pixel list into (scenes without soft lights): their sizes in pixels."""
    budget = (5 if host_classified else 2) * chunk_samples
    per = max(1, min(n_pix, budget // spp))
    if per > 64:
        n_chunks = (n_pix + per - 1) // per
        even = ((n_pix + n_chunks - 1) // n_chunks + 63) // 64 * 64
        per -= per % 64
        per = min(per, even)
    return [min(per, n_pix - p0) for p0 in range(0, n_pix, per)]


def group_log2(spp, wave_samples=0):
    """Samples per bounce-0 wavefront of a pass, as plan_chunks decides it: the largest power of two in spp, 2^4 (or the option) at most."""
    most, g = (wave_samples if wave_samples > 0 else 16), 0
    while (2 << g) <= most and not ((spp >> g) & 1):
        g += 1
    return g


# -------------------------------------------------------------------------------------------------- scenes, built through the API
W, H = 64, 32
COLOURS = ((0.3, 0.7, 0.1), (0.7, 0.1, 0.3), (0.1, 0.3, 0.7))     # non-dyadic: their squares and sums round


def edges_camera():
    """Straight down on the plane y = 0 from 10 above it: 8 pixels per unit, x in [-4, 4] over the 64 columns, z from 2 down to -2 over
    the 32 rows.  The reference divides the image plane's height by res_h - 1 and its width by res_v - 1 and starts at minus half the
    width (Image.fs:71-72), so the plane is sized for 63 x 31 pixels of 1/80 and the camera stands where column 15.5, row 31.5 look down."""
    pixel = 1.0 / 80.0
    height, width = (W - 1) * pixel, (H - 1) * pixel
    x, z = -4.0 + 10.0 * width / 2.0, -2.0 + 10.0 * (H * pixel - height / 2.0)
    return ft.make_camera((x, 10.0, z), (x, 0.0, z), (0.0, 0.0, 1.0), 2.0 * math.atan(height / 2.0), width / height)


def _square(b, x0, z0, side, colour, y=0.0, **material):
    return b.material(b.transform([("scale", (side, 1.0, side)), ("translate", (x0, y, z0))], b.primitive(ft.SQUARE)), colour=colour, **material)


def build_edges(b, with_nan=False):
    """Unlit squares over a black background under one directional light (an unlit surface emits its colour once per light): a pixel's
    samples are its square's colour or black, whole blocks inside a square are flat, and the scene is bounded, so the host classifies and
    k_classify finishes background blocks.  with_nan: a small lit square above the plane whose specular exponent is NaN."""
    b.clear()
    items = [_square(b, -3.3, -1.4, 2.7, COLOURS[0], apply_lighting=False),
             _square(b, -0.2, -0.7, 0.9, COLOURS[1], apply_lighting=False),
             _square(b, 0.55, 0.45, 0.8, COLOURS[2], apply_lighting=False)]
    if with_nan:
        items.append(_square(b, 1.7, -1.6, 0.3, (0.5, 0.5, 0.5), y=0.5, shineyness=float("nan")))
    b.set_objects(b.group(items))
    b.add_directional((0.3, -1.0, 0.2), (1.0, 1.0, 1.0))
    b.commit()
    return edges_camera()


def build_lit(b):
    """A lit sphere on a lit plane under one directional light: the shading varies inside every pixel of the sphere (continuous noise);
    the plane is unbounded, so the host does not classify and adaptive passes are mask-only."""
    b.clear()
    sphere = b.material(b.translate((0.0, 1.0, 0.0), b.primitive(ft.SPHERE)), colour=(0.9, 0.4, 0.2), shineyness=12.0)
    ground = b.material(b.primitive(ft.PLANE), colour=(0.3, 0.6, 0.7))
    b.set_objects(b.group([sphere, ground]))
    b.add_directional((-0.4, -1.0, 0.5), (1.0, 0.9, 0.8))
    b.commit()
    return ft.make_camera((0.0, 1.6, -4.5), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0), math.radians(38.0), W / H)


def single_sample_frames(ctx, cam, jit, w=W, h=H, seed=7):
    """The device's (or the oracle's) own frames of one sample each: by the header's exactness rule the samples a pass traces."""
    return [ctx.render(cam, w, h, 1, jit[k:k + 1], seed=seed)[0] if seed is not None else ctx.render(cam, w, h, 1, jit[k:k + 1])[0]
            for k in range(len(jit))]


def block_kinds(frames):
    """Per block of a run of single-sample frames: flat (every pixel took one value in every frame, not all black), background (all
    black), two_valued (some pixel took two values, none more)."""
    stack = np.stack(frames)                                        # [K, h, w, 3]
    same = np.all(stack == stack[:1], axis=0).all(axis=2)           # pixel: one value over the frames
    black = np.all(stack == 0.0, axis=(0, 3))
    two = np.zeros(same.shape, dtype=bool)
    more = np.zeros(same.shape, dtype=bool)
    for y, x in zip(*np.nonzero(~same)):
        k = len({tuple(v) for v in stack[:, y, x, :]})
        two[y, x], more[y, x] = k == 2, k > 2
    b = lambda m: per_block(m[..., None])
    return {"flat": b(same).all(axis=2) & ~b(black).all(axis=2), "background": b(black).all(axis=2),
            "two_valued": b(two).any(axis=2) & ~b(more).any(axis=2)}


# ----------------------------------------------------------------------------------- exact models of one pixel's arithmetic (CPU)
def fma(a, b, c):
    """a * b + c rounded once (Fraction.__float__ rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def se_rounded_apart(samples):
    """One channel's se after these samples, every operation rounded on its own (Python floats: the twin's arithmetic)."""
    S = Q = 0.0
    for c in samples:
        S = S + c
        cc = c * c
        Q = Q + cc
    n = float(len(samples))
    m = S / n
    mm = m * m
    v0 = Q / n - mm
    v = (0.0 if v0 < 0.0 else v0) * n / (n - 1.0)
    return math.sqrt(v / n), v0


def se_contracted(samples):
    """The same with the two contractions the device code had under -ffp-contract=on: Q = fma(c, c, Q), v0 = fma(-m, m, Q / n)."""
    S = Q = 0.0
    for c in samples:
        S = S + c
        Q = fma(c, c, Q)
    n = float(len(samples))
    m = S / n
    v0 = fma(-m, m, Q / n)
    v = (0.0 if v0 < 0.0 else v0) * n / (n - 1.0)
    return math.sqrt(v / n), v0


def exact_se_squared(S, Q, n):
    """The header's se^2 = max(0, Q/n - (S/n)^2) / (n - 1) of the doubles S, Q and the integer n, as a Fraction; and Q/n - (S/n)^2."""
    v0 = Fraction(Q) / n - (Fraction(S) / n) ** 2
    return max(Fraction(0), v0) / (n - 1), v0


def se_error_bound(S, Q, n):
    """A bound on |twin se - exact se| (see test_twin_against_exact_fractions for the derivation), as a Fraction, from the exact values."""
    se2, v0 = exact_se_squared(S, Q, n)
    u, eta = Fraction(U), Fraction(ETA)
    delta = Fraction(101, 100) * u * (abs(Fraction(Q)) / n + 3 * (Fraction(S) / n) ** 2 + abs(v0)) + (4 + 2 * (n - 1)) * eta
    return se2, Fraction(delta, n - 1)

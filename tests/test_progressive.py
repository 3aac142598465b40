"""Progressive accumulation (ft_progressive_*, include/functracer_hip.h): passes over pieces of a jitter pattern give the frame one ft_render
over the whole pattern gives, bit for bit; adaptive passes stop tracing 8x8 blocks whose pixels have settled."""
import ctypes as C

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from functracer_amd._capi import FtError
from oracle import ft_oracle_py as O

from . import helpers as H
from . import progressive_tools as T

PIECES = [1, 3, 4, 8]


def _load(ctx, name):
    p = ft.parse_scene_file(H.scene_path(name))
    p.lower(ctx)
    return p


def _split(jit, sizes):
    out, at = [], 0
    for k in sizes:
        out.append(jit[at:at + k])
        at += k
    return out


def _stderr(S, Q, n):
    """Standard error of the mean per channel as the header defines it (0 where fewer than 2 samples)."""
    dn = np.maximum(n, 1).astype(np.float64)[..., None]
    m = S / dn
    v0 = Q / dn - m * m
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(v0 < 0.0, 0.0, v0) * dn / (dn - 1.0)
        se = np.sqrt(v / dn)
    return np.where((n >= 2)[..., None], se, 0.0)


def _simulate(frames, tol, min_samples):
    """Adaptive accumulation of single-sample frames in numpy: per pass the running S, Q, n, the retired blocks, the pixels traced and the
    smallest relative distance of a deciding block's largest standard error from the tolerance."""
    h, w = frames[0].shape[:2]
    S, Q, n = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.int64)
    retired = np.zeros((h // 8, w // 8), dtype=bool)
    out = []
    for c in frames:
        live = ~np.repeat(np.repeat(retired, 8, 0), 8, 1)
        traced = int(live.sum())
        S = np.where(live[..., None], S + c, S)
        Q = np.where(live[..., None], Q + c * c, Q)
        n = np.where(live, n + 1, n)
        block_se = _stderr(S, Q, n).reshape(h // 8, 8, w // 8, 8, 3).max(axis=(1, 3, 4))
        deciding = ~retired & (n[::8, ::8] >= min_samples)
        margin = float(np.min(np.abs(block_se[deciding] - tol)) / tol) if deciding.any() and tol > 0 else np.inf
        retired = retired | (deciding & (block_se <= tol))
        out.append({"S": S, "Q": Q, "n": n, "retired": retired.copy(), "traced": traced, "margin": margin})
    return out


def _single_sample_frames(hip, cam, w, h, jit, seed=7):
    return [hip.render(cam, w, h, 1, jit[k:k + 1], seed=seed)[0] for k in range(len(jit))]


def _pick_tolerance(frames, min_samples):
    """A tolerance that retires some blocks early and leaves others active to the end, with no deciding block within 1e-6 of it."""
    free = _simulate(frames, 0.0, min_samples)[-1]
    block_se = _stderr(free["S"], free["Q"], free["n"]).reshape(frames[0].shape[0] // 8, 8, frames[0].shape[1] // 8, 8, 3).max(axis=(1, 3, 4))
    spread = np.sort(block_se[np.isfinite(block_se) & (block_se > 0)])
    assert spread.size > 4, "the scene has too few noisy blocks for an adaptive test"
    spread = np.unique(spread)
    for q in (0.5, 0.4, 0.6, 0.3, 0.7, 0.2, 0.8):
        i = int(q * (spread.size - 2))
        tol = float(0.5 * (spread[i] + spread[i + 1]))             # between two blocks' final errors
        sim = _simulate(frames, tol, min_samples)
        if min(s["margin"] for s in sim) > 1e-6 and sim[-1]["retired"].any() and not sim[-1]["retired"].all():
            return tol, sim
    raise AssertionError("no tolerance with a clear margin")


# ------------------------------------------------------------------------------------------------------------------------- CPU
def test_host_only_context_has_no_progressive_render():
    ctx = ft.Context(host_only=True)
    lib, h = ctx._lib, ctx._ctx
    cam = ft.make_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), 0.8)
    jit = np.zeros((1, 2))
    out, st = np.zeros((8, 8, 3)), _capi.ft_stats()
    assert lib.ft_progressive_begin(h, C.byref(cam), 8, 8, 8, None, 0, 0.0, 2) == -2
    assert lib.ft_progressive_begin(h, C.byref(cam), 8, 8, 8, None, 0, 0.01, 2) == -2
    assert lib.ft_progressive_pass(h, 1, _capi.dptr(jit), 1, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) == -2
    assert lib.ft_progressive_fetch(h, _capi.dptr(out), None, None) == -2
    assert lib.ft_progressive_status(h, (C.c_int64 * 6)()) == -2
    assert lib.ft_progressive_end(h) == -2
    with pytest.raises(FtError, match="NO_DEVICE"):
        ctx.progressive_begin(cam, 8, 8)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "night-house-det", "hollow-sphere", "sample-det", "bunny-bsp12"])
def test_passes_equal_the_one_shot_frame(hip, name):
    """After every pass the running mean is ft_render of the pattern so far, bit for bit, as FP64 and as RGBA8; plain accumulation
    retires nothing."""
    p = _load(hip, name)
    w, h = 96, 64
    jit = ft.jitter_pattern(sum(PIECES))
    done = 0
    for k, (frame, st) in enumerate(hip.progressive(p.camera, w, h, _split(jit, PIECES), [5] * len(PIECES))):
        done += PIECES[k]
        want, _ = hip.render(p.camera, w, h, done, jit[:done], seed=5)
        assert np.array_equal(frame, want), f"{name}: pass {k} differs from the one-shot frame of {done} samples"
        assert st["rays_primary"] == w * h * PIECES[k]
        status = hip.progressive_status()
        assert status == {"passes": k + 1, "min_samples": done, "max_samples": done, "blocks": w * h // 64, "blocks_retired": 0,
                          "samples_traced": status["samples_traced"]}
        assert 0 < status["samples_traced"] <= w * h * PIECES[k]
    mean, se, samples = hip.progressive_fetch()
    assert np.array_equal(mean, want) and se is None and (samples == done).all()
    done = 0
    for k, (u8, _) in enumerate(hip.progressive(p.camera, w, h, _split(jit, PIECES), [5] * len(PIECES), rgba8=True)):
        done += PIECES[k]
        want8, _ = hip.render_rgba8(p.camera, w, h, done, jit[:done], seed=5)
        assert np.array_equal(u8, want8), f"{name}: RGBA8 pass {k}"
    hip.progressive_end()


@pytest.mark.gpu
def test_tiles_and_interleaved_renders(hip):
    """An accumulation over two tiles (one of whole 8x8 blocks, one row-major) writes only their pixels; ft_render calls with another
    camera between the passes change nothing accumulated and render as on a fresh context (the pass forgets the zero-fill state)."""
    p = _load(hip, "bunny")
    w, h = 160, 96
    tiles = [(32, 16, 96, 64), (4, 70, 30, 13)]
    o = np.array(list(p.camera.o))
    back = o - (np.array(list(p.camera.look_at)) - o)
    other = ft.make_camera(o, back, list(p.camera.up), p.camera.fov_y, p.camera.aspect_ratio)   # facing away: every block finished
    fresh = ft.Context(device=0)
    try:
        _load(fresh, "bunny")
        want_other, _ = fresh.render(other, w, h, 2, ft.jitter_pattern(2), seed=3)
        jit = ft.jitter_pattern(8)
        hip.progressive_begin(p.camera, w, h, tiles=tiles)
        done = 0
        for k, piece in enumerate(_split(jit, [2, 2, 4])):
            got_other, _ = hip.render(other, w, h, 2, ft.jitter_pattern(2), seed=3)
            assert np.array_equal(got_other, want_other), f"interleaved render before pass {k}"
            out = np.full((h, w, 3), -1.0)
            hip.progressive_pass(len(piece), piece, seed=3, out=out)
            done += len(piece)
            want, _ = fresh.render(p.camera, w, h, done, jit[:done], seed=3, tiles=tiles)
            inside = np.zeros((h, w), dtype=bool)
            for x0, y0, tw, th in tiles:
                inside[y0:y0 + th, x0:x0 + tw] = True
            assert np.array_equal(out[inside], want[inside]), f"pass {k}"
            assert (out[~inside] == -1.0).all(), "a pixel outside the tiles was written"
            assert (out[inside] != 0).any()
        mean, _, samples = hip.progressive_fetch()
        assert np.array_equal(mean[inside], want[inside]) and (mean[~inside] == 0).all()
        assert (samples[inside] == 8).all() and (samples[~inside] == 0).all()
        assert np.array_equal(hip.render(other, w, h, 2, ft.jitter_pattern(2), seed=3)[0], want_other)
        hip.progressive_end()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_seeded_streams_of_passes(hip):
    """Soft lights and depth of field: a pass's samples are those of ft_render of that pass with its own seed, so passes of one sample
    average to the sequential numpy sum of those single-sample frames."""
    p = _load(hip, "sample-soft")
    assert p.camera.has_focus
    w, h = 64, 64
    jit = ft.jitter_pattern(5)
    seeds = [101, 202, 303, 404, 505]
    S = 0.0
    for k, (frame, _) in enumerate(hip.progressive(p.camera, w, h, [jit[k:k + 1] for k in range(5)], seeds)):
        c, _ = hip.render(p.camera, w, h, 1, jit[k:k + 1], seed=seeds[k])
        S = S + c
        assert np.array_equal(frame, S / (k + 1)), f"pass {k}"
    hip.progressive_end()


@pytest.mark.gpu
def test_adaptive_retirement(hip):
    """Passes of one sample on night-house-det (a ground plane: the frame is classified by the retired blocks only) with min_samples 4:
    the sample counts match numpy and the standard errors the exact twin bit for bit, the retired blocks are the criterion's, each block's mean is ft_render of its own
    prefix of the pattern, retired pixels never change again and the samples traced fall as blocks retire."""
    p = _load(hip, "night-house-det")
    w, h, K, min_samples = 96, 64, 16, 4
    jit = ft.jitter_pattern(K)
    frames = _single_sample_frames(hip, p.camera, w, h, jit)
    tol, sim = _pick_tolerance(frames, min_samples)
    twin = T.accumulate(frames, [1] * K, tol, min_samples)          # the exact twin (tests/progressive_tools.py), written apart from _simulate
    hip.progressive_begin(p.camera, w, h, tolerance=tol, min_samples=min_samples)
    means, traced = [], []
    for k in range(K):
        frame, _ = hip.progressive_pass(1, jit[k:k + 1], seed=7)
        means.append(frame)
        status = hip.progressive_status()
        traced.append(status["samples_traced"])
        want = sim[k]
        mean, se, samples = hip.progressive_fetch()
        assert np.array_equal(samples, want["n"]), f"pass {k}: samples per pixel"
        assert np.array_equal(mean, want["S"] / want["n"][..., None]) and np.array_equal(frame, mean), f"pass {k}: mean"
        assert np.array_equal(se, twin[k]["se"]), f"pass {k}: standard errors"                 # to the bit: the device rounds every operation apart
        assert status["blocks_retired"] == int(want["retired"].sum()) and status["passes"] == k + 1
        assert status["min_samples"] == want["n"].min() and status["max_samples"] == want["n"].max()
        assert traced[k] == want["traced"], f"pass {k}: samples traced"
    final = sim[-1]
    assert 0 < final["retired"].sum() < final["retired"].size
    assert traced[-1] < traced[0] == w * h
    for n in np.unique(final["n"]):                                 # each block: ft_render of its own prefix
        want, _ = hip.render(p.camera, w, h, int(n), jit[:n], seed=7)
        sel = final["n"] == n
        assert np.array_equal(means[-1][sel], want[sel]), f"blocks of {n} samples"
    for k in range(min_samples, K):                                 # retired pixels keep their mean
        gone = np.repeat(np.repeat(sim[k - 1]["retired"], 8, 0), 8, 1)
        assert np.array_equal(means[k][gone], means[k - 1][gone]), f"pass {k}: a retired pixel changed"
    hip.progressive_end()


@pytest.mark.gpu
def test_multi_device_accumulation_equals_single_device(hip):
    """Every device accumulates and retires its 8-row bands; fetch and status combine them into the single device's state."""
    import torch
    n_dev = torch.cuda.device_count()
    ordinals = list(range(min(n_dev, 4))) if n_dev > 1 else [0, 0, 0]
    p = _load(hip, "night-house-det")
    multi = ft.Context(device=ordinals)
    try:
        p.lower(multi)
        w, h, K = 96, 64, 10
        jit = ft.jitter_pattern(K)
        frames = _single_sample_frames(hip, p.camera, w, h, jit)
        tol, _ = _pick_tolerance(frames, 4)
        for tolerance, sizes in ((0.0, [1, 2, 3, 4]), (tol, [1] * K)):
            results = []
            for ctx in (hip, multi):
                frames_out = [f for f, _ in ctx.progressive(p.camera, w, h, _split(jit, sizes), list(range(len(sizes))), tolerance=tolerance, min_samples=4)]
                results.append((frames_out, ctx.progressive_fetch(), ctx.progressive_status()))
                ctx.progressive_end()
            (f1, (m1, s1, n1), st1), (f2, (m2, s2, n2), st2) = results
            assert all(np.array_equal(a, b) for a, b in zip(f1, f2)), f"tolerance {tolerance}: frames"
            assert np.array_equal(m1, m2) and np.array_equal(n1, n2) and st1 == st2, f"tolerance {tolerance}: state"
            assert (s1 is None and s2 is None) or np.array_equal(s1, s2)
            assert (st1["blocks_retired"] > 0) == (tolerance > 0)
    finally:
        multi.close()


@pytest.mark.gpu
def test_accumulated_frame_against_the_oracle(hip):
    p = _load(hip, "hollow-sphere")
    orc = O.Oracle()
    p.lower(orc)
    w, h = 64, 48
    jit = ft.jitter_pattern(4)
    for frame, _ in hip.progressive(p.camera, w, h, _split(jit, [1, 3]), [1, 2]):
        pass
    want, _ = orc.render(p.camera, w, h, 4, jit)
    assert H.assert_frames_match(frame, want, what="progressive hollow-sphere") < 1e-9
    hip.progressive_end()


@pytest.mark.gpu
def test_overflow_during_a_pass(hip):
    """A mesh under CSG at a capacity of 2 hits: a pass that overflows leaves no trace (with csg_auto_grow off it fails and nothing is
    accumulated); with growth on, the lists grow, the scene is committed again, the accumulation survives and the pass counts once."""
    tris = np.asarray(ft.parse_ply(open(H.scene_path("meshes/bunny_synth_res4").replace(".scene", ".ply")).read())).reshape(-1, 9)
    cam = ft.make_camera((0, 1, -6), (0, 0.6, 0), (0, 1, 0), H.deg(40.0))
    jit = ft.jitter_pattern(4)
    try:
        hip.set_option("csg_mesh_capacity", 2)
        hip.set_option("csg_auto_grow", 0)
        hip.clear()
        m = hip.scale(7.0, hip.bsp_mesh(3, tris))
        node = hip.subtract(m, hip.translate((0.0, 0.9, -0.3), hip.scale(0.5, hip.primitive(ft.SPHERE))))
        hip.set_objects(hip.group([hip.material(node, colour=(0.8, 0.5, 0.3), reflectance=0.2, shineyness=10)]))
        hip.add_directional((-1, -1, 1), (1, 1, 1))
        hip.commit()
        small = hip.scene_info()["csg_capacity"]
        hip.progressive_begin(cam, 96, 64)
        with pytest.raises(FtError, match="OVERFLOW"):
            hip.progressive_pass(1, jit[:1], seed=1)
        status = hip.progressive_status()
        assert status["passes"] == 0 and status["max_samples"] == 0
        hip.set_option("csg_auto_grow", 1)
        first, st = hip.progressive_pass(1, jit[:1], seed=1)
        assert hip.scene_info()["csg_capacity"] > small and st["csg_overflow"] == 0
        second, _ = hip.progressive_pass(3, jit[1:4], seed=1)
        status = hip.progressive_status()
        assert status["passes"] == 2 and status["min_samples"] == status["max_samples"] == 4
        assert np.array_equal(first, hip.render(cam, 96, 64, 1, jit[:1], seed=1)[0])
        assert np.array_equal(second, hip.render(cam, 96, 64, 4, jit, seed=1)[0])
        hip.progressive_end()
    finally:
        hip.set_option("csg_auto_grow", 1)
        hip.set_option("csg_mesh_capacity", 32)


@pytest.mark.gpu
def test_progressive_errors(hip):
    p = _load(hip, "bunny")
    jit = ft.jitter_pattern(2)
    hip.progressive_end()
    with pytest.raises(FtError, match="STATE"):                     # no begin
        hip.progressive_pass(1, jit[:1])
    assert hip._lib.ft_progressive_pass(hip._ctx, 1, _capi.dptr(jit), 1, 0, None, None) == -5
    assert hip._lib.ft_progressive_status(hip._ctx, (C.c_int64 * 6)()) == -5
    hip.progressive_begin(p.camera, 64, 64)
    with pytest.raises(FtError, match="UNSUPPORTED"):               # corner sampling
        hip.progressive_pass(0, None)
    hip.progressive_pass(1, jit[:1])
    p.lower(hip)                                                    # the caller's commit ends the accumulation
    with pytest.raises(FtError, match="STATE"):
        hip.progressive_pass(1, jit[1:])
    with pytest.raises(FtError, match="STATE"):
        hip.progressive_status()
    with pytest.raises(FtError, match="UNSUPPORTED"):               # adaptive mode retires whole 8x8 blocks
        hip.progressive_begin(p.camera, 100, 60, tolerance=0.01, min_samples=4)
    with pytest.raises(FtError, match="INVALID"):
        hip.progressive_begin(p.camera, 64, 64, tolerance=0.01, min_samples=1)
    hip.progressive_begin(p.camera, 100, 60)                        # plain accumulation takes any frame
    frame, _ = hip.progressive_pass(2, jit)
    assert np.array_equal(frame, hip.render(p.camera, 100, 60, 2, jit)[0])
    with pytest.raises(FtError, match="STATE"):                     # no standard errors without an adaptive accumulation
        hip._check(hip._lib.ft_progressive_fetch(hip._ctx, None, _capi.dptr(np.zeros((60, 100, 3))), None))
    hip.progressive_end()
    with pytest.raises(FtError, match="STATE"):
        hip.progressive_pass(1, jit[:1])

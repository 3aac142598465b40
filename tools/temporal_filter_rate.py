#!/usr/bin/env python3
"""ft_temporal_filter behind ft_temporal_accumulate(to_frame) along an orbit of `frames` calls (0.5 degrees per call) at 1920x1080 on
bunny, night-house and moon, 1-spp frames, the result leaving as RGBA8 into page-locked memory (one of `out` and `out_variance` has to be
given).  Per call of the orbit three filter calls, all with sigma_position on so that a tap reads all of its 81 B: no iterations and no
demodulation (its kernel time is k_tfilter_prepare's), N iterations without demodulation (minus the former: the iterations) and N
iterations with demodulation (the guide pass k_aov is reported as trace_kernel_ms; the scatter is the remainder).  "rest" is the call's
wall time minus its kernel time.  Bytes by construction per frame pixel: k_tfilter_prepare reads M, Q, N, leaf and the class (61) and
writes class, u_0 and v_0 (33): 94; an iteration reads class, n, p, u and v (81) and writes u and v (32): 113; the other 24 + 8 taps
are re-reads.  Medians over the calls after the first two.  Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from temporal_rate import orbit

PREPARE_BYTES, ITERATION_BYTES = 94, 113


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res_h, res_v = 1920, 1080
    jit = np.zeros((1, 2))
    kw = dict(sigma_colour=2.0, sigma_normal=0.3, sigma_position=1.0, min_history=4)
    out = {"res": [res_h, res_v], "frames": frames, "iterations": iterations, "bytes_per_pixel": {"prepare": PREPARE_BYTES, "iteration": ITERATION_BYTES}}
    med = lambda v: statistics.median(v)
    with ft.PinnedArray((res_v, res_h, 4), dtype=np.uint8) as rgba:
        for name in ("bunny", "night-house", "moon"):
            wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
            ctx = ft.Context(0)
            wl.lower(ctx)
            ctx.temporal_begin(res_h, res_v)
            prepare, iters, rest_plain, rest_demod, aov, scatter, short = [], [], [], [], [], [], []
            for k in range(frames + 2):
                cam = orbit(wl.camera, k)
                ctx.render(cam, res_h, res_v, 1, jit, seed=k, fetch=False)
                ctx.temporal_accumulate(cam, 1, jit, seed=k, to_frame=1, fetch=False)
                _, _, s0 = ctx.temporal_filter(rgba8=True, out=rgba, demodulate=0, iterations=0, **kw)
                _, _, s1 = ctx.temporal_filter(rgba8=True, out=rgba, demodulate=0, iterations=iterations, **kw)
                _, _, s2 = ctx.temporal_filter(cam, 1, jit, seed=k, rgba8=True, out=rgba, demodulate=1, iterations=iterations, **kw)
                if k >= 2:
                    prepare.append(s0["kernel_ms"]); iters.append(s1["kernel_ms"] - s0["kernel_ms"])
                    rest_plain.append(s1["wall_ms"] - s1["kernel_ms"]); rest_demod.append(s2["wall_ms"] - s2["kernel_ms"])
                    aov.append(s2["trace_kernel_ms"]); scatter.append(s2["kernel_ms"] - s2["trace_kernel_ms"] - s1["kernel_ms"])
            n_px = res_h * res_v
            out[name] = {"k_tfilter_prepare_ms": round(med(prepare), 4), "iterations_ms": round(med(iters), 4),
                         "prepare_bytes_by_construction_GBps": round(PREPARE_BYTES * n_px / (med(prepare) * 1e-3) / 1e9, 1),
                         "iterations_bytes_by_construction_GBps": round(iterations * ITERATION_BYTES * n_px / (med(iters) * 1e-3) / 1e9, 1),
                         "k_aov_ms": round(med(aov), 4), "k_tfilter_scatter_ms": round(med(scatter), 4),
                         "rest_of_call_ms": round(med(rest_plain), 3), "rest_of_call_demodulate_ms": round(med(rest_demod), 3)}
            ctx.temporal_end()
            ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

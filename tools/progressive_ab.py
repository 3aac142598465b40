#!/usr/bin/env python3
"""One blocking ft_render at N spp against N / k progressive passes of k spp (ft_progressive_*), plain and adaptive: ms per pass, total ms
and samples traced.  Frames stay in HBM (no PCIe copy is timed).  Each variant runs --repeats times; the medians are reported.  Also: one
ft_render at k spp (what a pass would cost without the running sums) and, with option "timing" = 2, the stage times of one such render
and of one plain pass (k_resolve against k_resolve_progressive).

python tools/progressive_ab.py --scene bunny --res 1920x1080 --spp 16 --per-pass 16
python tools/progressive_ab.py --scene night-house-det --res 1920x1080 --spp 64 --per-pass 4 --tolerance 0.00392156862745098 --min-samples 8
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import functracer_amd as ft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bunny")
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16, help="N: samples per pixel of the whole frame")
    ap.add_argument("--per-pass", type=int, default=16, help="k: samples per progressive pass")
    ap.add_argument("--tolerance", type=float, default=0.0, help="> 0: also run the adaptive form with this tolerance")
    ap.add_argument("--min-samples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    w, h = (int(v) for v in a.res.split("x"))
    assert a.spp % a.per_pass == 0, "--spp must be a multiple of --per-pass"
    p = ft.parse_scene_file(os.path.join(ROOT, "scenes", a.scene + ".scene"))
    ctx = ft.Context(device=0)
    p.lower(ctx)
    jit = ft.jitter_pattern(a.spp)
    pieces = [jit[i:i + a.per_pass] for i in range(0, a.spp, a.per_pass)]
    seed = ft.DEFAULT_SEED

    def one_shot(n=a.spp):
        t0 = time.perf_counter()
        _, st = ctx.render(p.camera, w, h, n, jit[:n], seed=seed, fetch=False)
        return {"total_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st["kernel_ms"], "samples_traced": st["rays_primary"] - st["rays_primary_culled"]}

    def passes(tolerance):
        ctx.progressive_begin(p.camera, w, h, tolerance=tolerance, min_samples=a.min_samples)
        per_pass, traced, kernel = [], [], []
        for k, piece in enumerate(pieces):
            t0 = time.perf_counter()
            _, st = ctx.progressive_pass(len(piece), piece, seed=seed + k, fetch=False)
            per_pass.append((time.perf_counter() - t0) * 1e3)
            kernel.append(st["kernel_ms"])
            traced.append(st["rays_primary"] - st["rays_primary_culled"])   # = ft_progressive_status' samples traced, without a call between passes
        status = ctx.progressive_status()
        ctx.progressive_end()
        return {"total_ms": sum(per_pass), "ms_per_pass": per_pass, "kernel_ms_per_pass": kernel, "samples_traced": sum(traced),
                "samples_traced_per_pass": traced, "blocks": status["blocks"], "blocks_retired": status["blocks_retired"],
                "min_samples": status["min_samples"], "max_samples": status["max_samples"]}

    def median_of(fn, *args):
        fn(*args)                                                   # warm-up (buffers, code objects)
        runs = [fn(*args) for _ in range(a.repeats)]
        out = dict(runs[len(runs) // 2])
        out["total_ms"] = statistics.median(r["total_ms"] for r in runs)
        out["total_ms_all"] = [round(r["total_ms"], 4) for r in runs]
        if "ms_per_pass" in out:
            out["ms_per_pass"] = [round(statistics.median(r["ms_per_pass"][i] for r in runs), 4) for i in range(len(pieces))]
            out["kernel_ms_per_pass"] = [round(statistics.median(r["kernel_ms_per_pass"][i] for r in runs), 4) for i in range(len(pieces))]
        return out

    result = {"scene": a.scene, "res": [w, h], "spp": a.spp, "per_pass": a.per_pass, "passes": len(pieces), "repeats": a.repeats,
              "one_shot": median_of(one_shot), "render_per_pass": median_of(one_shot, a.per_pass), "progressive": median_of(passes, 0.0)}
    if a.tolerance > 0:
        result["adaptive"] = median_of(passes, a.tolerance)
        result["adaptive"].update(tolerance=a.tolerance, min_samples_to_retire=a.min_samples)
    ctx.set_option("timing", 2)                                     # stage times: an event around every kernel (costs ~6 us each)
    stages = {}
    for name in ("render", "pass"):
        for _ in range(2):                                          # the second of each: warm, and the same zero-fill state as the timed loop
            if name == "render":
                ctx.render(p.camera, w, h, a.per_pass, pieces[0], seed=seed, fetch=False)
            else:
                ctx.progressive_begin(p.camera, w, h)
                ctx.progressive_pass(a.per_pass, pieces[0], seed=seed, fetch=False)
                ctx.progressive_end()
        stages[name] = {k: round(v["ms"], 4) for k, v in ctx.kernel_times().items()}
    ctx.set_option("timing", 1)
    result["stage_ms_timing2"] = stages
    result["progressive_over_one_shot"] = round(result["progressive"]["total_ms"] / result["one_shot"]["total_ms"], 4)
    if "adaptive" in result:
        result["adaptive_over_one_shot"] = round(result["adaptive"]["total_ms"] / result["one_shot"]["total_ms"], 4)
    result["pass_over_render_per_pass"] = round(statistics.median(result["progressive"]["ms_per_pass"]) / result["render_per_pass"]["total_ms"], 4)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

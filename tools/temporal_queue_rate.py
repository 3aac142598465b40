#!/usr/bin/env python3
"""ft_temporal_enqueue against the blocking pair: an orbit of 0.5 degrees per call at 1920x1080 on night-house and bunny,
1-spp frames, the filtered history (4 iterations, without and with demodulate) leaving as RGBA8 into a ring of four page-locked buffers.
  A  blocking: ft_render(out NULL), ft_temporal_accumulate(out NULL), ft_temporal_filter(rgba8 -> pinned), per frame
  B  queued:   ft_render_enqueue, ft_temporal_enqueue(filter, rgba8 -> pinned), per frame; one ft_temporal_wait at the end
`frames` frames per series behind two untimed ones, the series interleaved (A B A B per form), the whole run `runs` times in fresh
contexts.  Per scene and form: wall time per frame of A and B per run, their median and range, B / A, and the kernel time per frame - A's
from the three calls' kernel_ms, B's from a stepped pass that waits after every call (the stats of a queued call arrive with the wait).
Prints one JSON line per scene and form; run on the GPU box."""
import json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from temporal_rate import orbit

RES = (1920, 1080)
WARM = 2


def blocking(ctx, wl, frames, filt, ring):
    w, h = RES
    jit = np.zeros((1, 2))
    ctx.temporal_begin(w, h)
    kernel = 0.0
    for k in range(WARM + frames):
        if k == WARM:
            t0, kernel = time.perf_counter(), 0.0
        cam = orbit(wl.camera, k)
        _, s0 = ctx.render(cam, w, h, 1, jit, seed=k, fetch=False)
        _, s1 = ctx.temporal_accumulate(cam, 1, jit, seed=k, fetch=False)
        _, _, s2 = ctx.temporal_filter(cam, 1, jit, seed=k, rgba8=True, out=ring[k % len(ring)], **filt)
        kernel += s0["kernel_ms"] + s1["kernel_ms"] + s2["kernel_ms"]
    wall = (time.perf_counter() - t0) * 1e3
    ctx.temporal_end()
    return wall / frames, kernel / frames


def queued(ctx, wl, frames, filt, ring, stepped=False):
    w, h = RES
    jit = np.zeros((1, 2))
    ctx.temporal_begin(w, h)
    kernel = 0.0
    for k in range(WARM + frames):
        if k == WARM:
            ctx.temporal_wait()
            ctx.wait()
            t0, kernel = time.perf_counter(), 0.0
        cam = orbit(wl.camera, k)
        ctx.render_enqueue(cam, w, h, 1, jit, seed=k)
        ctx.temporal_enqueue(cam, 1, jit, seed=k, rgba8=True, out=ring[k % len(ring)], filter=filt)
        if stepped:
            kernel += ctx.temporal_wait()["kernel_ms"] + ctx.wait()["kernel_ms"]
    ctx.temporal_wait()
    wall = (time.perf_counter() - t0) * 1e3
    ctx.wait()
    ctx.temporal_end()
    return wall / frames, kernel / frames


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    forms = {"filter": dict(iterations=4, demodulate=0), "filter+demodulate": dict(iterations=4, demodulate=1)}
    pinned = [ft.PinnedArray((RES[1], RES[0], 4), dtype=np.uint8) for _ in range(4)]
    ring = [p.array for p in pinned]
    rows = {}
    for run in range(runs):
        for name in ("night-house", "bunny"):
            wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
            ctx = ft.Context(0)
            wl.lower(ctx)
            for form, filt in forms.items():
                row = rows.setdefault((name, form), {"scene": name, "form": form, "res": list(RES), "frames": frames, "A_wall_ms": [], "B_wall_ms": [],
                                                     "A_kernel_ms": [], "B_kernel_ms": []})
                for _ in range(2):                                   # interleaved: A B A B
                    a = blocking(ctx, wl, frames, filt, ring)
                    b = queued(ctx, wl, frames, filt, ring)
                    row["A_wall_ms"].append(round(a[0], 4)); row["A_kernel_ms"].append(round(a[1], 4)); row["B_wall_ms"].append(round(b[0], 4))
                row["B_kernel_ms"].append(round(queued(ctx, wl, frames, filt, ring, stepped=True)[1], 4))
            ctx.close()
    for row in rows.values():
        a, b = row["A_wall_ms"], row["B_wall_ms"]
        row["A_median_range_ms"] = [round(statistics.median(a), 4), min(a), max(a)]
        row["B_median_range_ms"] = [round(statistics.median(b), 4), min(b), max(b)]
        row["B_over_A"] = round(statistics.median(b) / statistics.median(a), 4)
        row["B_below_A_beyond_its_spread"] = max(b) < min(a)
        row["B_wall_over_its_kernel_ms"] = round(statistics.median(b) - statistics.median(row["B_kernel_ms"]), 4)
        print(json.dumps(row))
    for p in pinned:
        p.close()


if __name__ == "__main__":
    main()

"""A/B of the per-frame overheads on the headline (GPU box): queued frames, wall ms per frame for every setting of
classify_ahead / zero_fill_skip / resolve_aside.  python tools/frame_overlap_ab.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
ctx = ft.Context(0); p = ft.parse_scene_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes/bunny.scene")); p.lower(ctx); jit = ft.jitter_pattern(16)
for ahead, skip, aside in ((0, 0, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1), (1, 0, 1)):
    ctx.set_option("classify_ahead", ahead); ctx.set_option("zero_fill_skip", skip); ctx.set_option("resolve_aside", aside)
    best = 1e9
    for rep in range(4):
        for _ in range(300): ctx.render_enqueue(p.camera, 1920, 1080, 16, jit)
        ctx.wait()
        t0 = time.perf_counter()
        for _ in range(200): ctx.render_enqueue(p.camera, 1920, 1080, 16, jit)
        ctx.wait(); best = min(best, (time.perf_counter() - t0) / 200 * 1e3)
    print(f"classify_ahead {ahead} zero_fill_skip {skip} resolve_aside {aside}: {best:.4f} ms/frame", {k: round(v["ms"] / 200, 4) for k, v in ctx.kernel_times().items() if v["ms"]})

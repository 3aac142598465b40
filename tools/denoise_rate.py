#!/usr/bin/env python3
"""ft_denoise at 1920x1080 (bunny, night-house, moon) and 3840x2160 (bunny), 5 iterations, 1-spp frames: the call's kernel time (guide
pass k_aov + k_denoise_scatter + the k_denoise iterations) and the rest of the call (the copy out), FP64 into pageable and into
page-locked memory and RGBA8 into page-locked memory, beside the 1-spp ft_render that made the frame.  Bytes by construction: the
scatter writes the 81-byte guide record and 24 bytes of u_0 and reads 76 + 24; an iteration reads 49 bytes of neighbour guides, 32 of
the pixel's own (d, V) and 24 of colour, and writes 24: 129 bytes per pixel once, everything else is re-reads.  Per-kernel times come
from a rocprofv3 --kernel-trace --stats run of this script.  Medians of `frames` calls.  Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft

ITERATION_BYTES = 49 + 32 + 24 + 24


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jit = np.zeros((1, 2))
    out = {"frames": frames, "iterations": 5, "iteration_bytes_per_pixel": ITERATION_BYTES}
    for name, res_h, res_v in (("bunny", 1920, 1080), ("night-house", 1920, 1080), ("moon", 1920, 1080), ("bunny", 3840, 2160)):
        wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
        ctx = ft.Context(0)
        wl.lower(ctx)
        cam = wl.camera
        _, st = ctx.render(cam, res_h, res_v, 1, jit, fetch=False)
        row = {"render_1spp_kernel_ms": round(st["kernel_ms"], 3)}
        with ft.PinnedArray((res_v, res_h, 3)) as pin64, ft.PinnedArray((res_v, res_h, 4), dtype=np.uint8) as pin8:
            for label, kw in (("fp64_pageable", {}), ("fp64_pinned", {"out": pin64}), ("rgba8_pinned", {"out": pin8, "rgba8": True}),
                              ("zero_iterations_fp64_pinned", {"out": pin64, "iterations": 0})):
                ks, rest = [], []
                for k in range(frames + 2):
                    _, st = ctx.denoise(cam, res_h, res_v, 1, jit, **{"iterations": 5, **kw})
                    if k >= 2:
                        ks.append(st["kernel_ms"]); rest.append(st["wall_ms"] - st["kernel_ms"])
                row[label] = {"kernel_ms": round(statistics.median(ks), 3), "rest_of_call_ms": round(statistics.median(rest), 3)}
        ms = row["fp64_pinned"]["kernel_ms"]
        row["all_kernels_bytes_by_construction_GBps"] = round((5 * ITERATION_BYTES + 81 + 24 + 76 + 24) * res_h * res_v / (ms * 1e-3) / 1e9, 1)
        out[f"{name}_{res_h}x{res_v}"] = row
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

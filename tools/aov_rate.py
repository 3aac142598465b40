#!/usr/bin/env python3
"""ft_render_aov against a blocking 1-spp ft_render of the same view (bunny, hollow-sphere at 1920x1080): k_aov's kernel time beside the
frame's k_primary time, and the rest of the AOV call (device-to-host copies of the planes and the host's scatter into frame layout) for
all channels (116 B per pixel) and for depth alone (8 B).  Medians of `frames` calls.  Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res_h, res_v = 1920, 1080
    jit = np.zeros((1, 2))
    out = {"res": [res_h, res_v], "frames": frames}
    for name in ("bunny", "hollow-sphere"):
        wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
        ctx = ft.Context(0)
        wl.lower(ctx)
        cam = wl.camera
        row = {}
        prim, frame_k, frame_wall = [], [], []
        for k in range(frames + 2):
            _, st = ctx.render(cam, res_h, res_v, 1, jit, fetch=False)
            if k >= 2:
                prim.append(ctx.kernel_times()["primary"]["ms"]); frame_k.append(st["kernel_ms"]); frame_wall.append(st["wall_ms"])
        row["render_1spp"] = {"k_primary_ms": round(statistics.median(prim), 3), "kernel_ms": round(statistics.median(frame_k), 3),
                              "wall_ms_no_fetch": round(statistics.median(frame_wall), 3)}
        for label, channels in (("aov_all", None), ("aov_t", ["t"])):
            ks, rest = [], []
            for k in range(frames + 2):
                st = ctx.render_aov(cam, res_h, res_v, 1, jit, channels=channels)["stats"]
                if k >= 2:
                    ks.append(st["kernel_ms"]); rest.append(st["wall_ms"] - st["kernel_ms"])
            row[label] = {"k_aov_ms": round(statistics.median(ks), 3), "copy_and_scatter_ms": round(statistics.median(rest), 3)}
        out[name] = row
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

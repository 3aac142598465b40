#!/usr/bin/env python3
"""What the neighbourhood clamp of ft_temporal_accumulate (ft_temporal_set_clamp) costs at 1920x1080: tools/temporal_rate.py's
orbit (0.5 degrees per call, 1-spp frames left in HBM, to_frame, nothing copied out) on bunny, night-house and moon, run by four contexts
side by side - the clamp off, and on with radius 1, 2 and 3 (gamma 1, floor 1e-4, clamped_history 1) - which take turns call by call, so
that whatever else the machine is doing reaches all four alike.  Per variant the call's kernel time without its guide pass (kernel_ms -
trace_kernel_ms: k_temporal, and with the clamp on k_temporal_box in front of it), as median and as smallest .. largest over the calls
after the first two; the kernels launched; the pixels clamped.  Bytes by construction per tile pixel: the clamp adds the frame's colour
once more (24) and the mask (1) in and the boxes (48) out in k_temporal_box (the halo's re-reads are cached), and the boxes (48) in again
in k_temporal: 121 B beside the 320 B of k_temporal and the 56 B of k_aov (4 + 52 out).
Writes profiles/temporal_clamp_rate.txt and the block between the two temporal_clamp_rate marks in DESIGN.md 12.1, and prints one JSON
line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import functracer_amd as ft
from temporal_rate import BYTES_PER_PIXEL, orbit

CLAMP_BYTES_PER_PIXEL = 24 + 1 + 48 + 48
VARIANTS = [("off", None), ("r1", 1), ("r2", 2), ("r3", 3)]
MARKS = ("<!-- temporal_clamp_rate: begin -->", "<!-- temporal_clamp_rate: end -->")


def measure(root, name, frames, res_h, res_v):
    wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
    jit = np.zeros((1, 2))
    ctxs = []
    for _, radius in VARIANTS:
        ctx = ft.Context(0)
        wl.lower(ctx)
        ctx.temporal_begin(res_h, res_v)
        if radius:
            ctx.temporal_set_clamp(radius=radius)
        ctxs.append(ctx)
    ms = [[] for _ in VARIANTS]
    launches, clamped, history = [0] * len(VARIANTS), [[] for _ in VARIANTS], []
    for k in range(frames + 2):
        cam = orbit(wl.camera, k)
        for v, ctx in enumerate(ctxs):
            ctx.render(cam, res_h, res_v, 1, jit, seed=k, fetch=False)
            _, ts = ctx.temporal_accumulate(cam, 1, jit, seed=k, to_frame=1, fetch=False)
            if k >= 2:
                ms[v].append(ts["kernel_ms"] - ts["trace_kernel_ms"])
                launches[v] = ts["n_launches"]
                clamped[v].append(ctx.temporal_clamp_status()["clamped"])
                if v == 0:
                    history.append(ctx.temporal_status()["with_history"])
    for ctx in ctxs:
        ctx.temporal_end()
        ctx.close()
    row = {"pixels_with_history": int(statistics.median(history))}
    for v, (tag, _) in enumerate(VARIANTS):
        row[tag] = {"ms_median": round(statistics.median(ms[v]), 4), "ms_min": round(min(ms[v]), 4), "ms_max": round(max(ms[v]), 4), "n_launches": launches[v],
                    "clamped_median": int(statistics.median(clamped[v]))}
    return row


def table(out):
    lines = [f"`tools/temporal_clamp_rate.py {out['frames']}`: {out['res'][0]}x{out['res'][1]}, the kernel time of a call without its guide pass in ms, median (smallest .. largest) "
             f"of {out['frames']} calls; the four variants take turns call by call.", "",
             "| frame | pixels with history | clamp off | r = 1 | r = 2 | r = 3 | clamped at r = 1, 2, 3 |", "|---|---|---|---|---|---|---|"]
    for name in out["scenes"]:
        r = out[name]
        cell = lambda t: f"{r[t]['ms_median']:.3f} ({r[t]['ms_min']:.3f} .. {r[t]['ms_max']:.3f})"
        lines.append(f"| {name} | {r['pixels_with_history']} | {cell('off')} | {cell('r1')} | {cell('r2')} | {cell('r3')} | "
                     f"{r['r1']['clamped_median']}, {r['r2']['clamped_median']}, {r['r3']['clamped_median']} |")
    lines += ["", f"Bytes by construction per tile pixel: {CLAMP_BYTES_PER_PIXEL} B more (colour 24 and mask 1 in, boxes 48 out, boxes 48 in again) beside "
              f"{BYTES_PER_PIXEL} B of `k_temporal` and 56 B of `k_aov`."]
    return "\n".join(lines)


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res_h, res_v = 1920, 1080
    out = {"res": [res_h, res_v], "frames": frames, "bytes_per_pixel": BYTES_PER_PIXEL, "clamp_bytes_per_pixel": CLAMP_BYTES_PER_PIXEL, "scenes": ["bunny", "night-house", "moon"]}
    for name in out["scenes"]:
        out[name] = measure(root, name, frames, res_h, res_v)
    text = table(out)
    with open(os.path.join(root, "profiles", "temporal_clamp_rate.txt"), "w") as f:
        f.write(text + "\n\n" + json.dumps(out) + "\n")
    design = os.path.join(root, "DESIGN.md")
    doc = open(design).read()
    if MARKS[0] in doc and MARKS[1] in doc:
        head, rest = doc.split(MARKS[0], 1)
        _, tail = rest.split(MARKS[1], 1)
        with open(design, "w") as f:
            f.write(head + MARKS[0] + "\n" + text + "\n" + MARKS[1] + tail)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

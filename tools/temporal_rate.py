#!/usr/bin/env python3
"""ft_temporal_accumulate along an orbit of `frames` calls (0.5 degrees per call) at 1920x1080 on bunny, night-house and moon, 1-spp
frames left in HBM (to_frame, nothing copied out): per call the time of k_temporal (the call's kernel time minus its guide pass k_aov,
which the call reports as trace_kernel_ms), of k_aov, the rest of the call, and the 1-spp ft_render that made the frame.  Bytes by
construction per tile pixel: k_temporal reads its list entry (4), k_aov's p, n and leaf of the window (52) and the frame's colour (24),
gathers one history record (108: each of the four taps of a pixel is also a tap of its neighbours, so a set is read once), and writes
the new record (108) and the result (24): 320 B; the other three taps are re-reads.  Medians over the calls after the first two (the
first has no history behind it).  Prints one JSON line; run on the GPU box."""
import json, math, os, statistics, sys
import ctypes as C
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from functracer_amd import _capi

BYTES_PER_PIXEL = 4 + 52 + 24 + 108 + 108 + 24


def orbit(cam, k, step_deg=0.5):
    """The eye circles the point it looks at about the y axis."""
    o, look = np.array(cam.o[:]), np.array(cam.look_at[:])
    a, v = math.radians(k * step_deg), o - look
    out = _capi.ft_camera.from_buffer_copy(cam)
    out.o = (C.c_double * 3)(look[0] + math.cos(a) * v[0] + math.sin(a) * v[2], look[1] + v[1], look[2] - math.sin(a) * v[0] + math.cos(a) * v[2])
    return out


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res_h, res_v = 1920, 1080
    jit = np.zeros((1, 2))
    out = {"res": [res_h, res_v], "frames": frames, "bytes_per_pixel": BYTES_PER_PIXEL}
    for name in ("bunny", "night-house", "moon"):
        wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
        ctx = ft.Context(0)
        wl.lower(ctx)
        ctx.temporal_begin(res_h, res_v)
        render, temporal, aov, rest, history = [], [], [], [], []
        for k in range(frames + 2):
            cam = orbit(wl.camera, k)
            _, st = ctx.render(cam, res_h, res_v, 1, jit, seed=k, fetch=False)
            _, ts = ctx.temporal_accumulate(cam, 1, jit, seed=k, to_frame=1, fetch=False)
            if k >= 2:
                render.append(st["kernel_ms"]); aov.append(ts["trace_kernel_ms"]); temporal.append(ts["kernel_ms"] - ts["trace_kernel_ms"])
                rest.append(ts["wall_ms"] - ts["kernel_ms"]); history.append(ctx.temporal_status()["with_history"])
        ms = statistics.median(temporal)
        out[name] = {"render_1spp_kernel_ms": round(statistics.median(render), 3), "k_aov_ms": round(statistics.median(aov), 3),
                     "k_temporal_ms": round(ms, 4), "k_temporal_bytes_by_construction_GBps": round(BYTES_PER_PIXEL * res_h * res_v / (ms * 1e-3) / 1e9, 1),
                     "rest_of_call_ms": round(statistics.median(rest), 3), "pixels_with_history": int(statistics.median(history))}
        ctx.temporal_end()
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

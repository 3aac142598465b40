#!/usr/bin/env python3
"""The period of a stream of queued headline-size frames (bunny, 1920x1080x16, left in HBM) in two series: `orbit`, every frame from
another camera (0.05 degrees per frame about the point looked at), so that no frame finds its slot's classification ("classify_reuse"
must cost such a stream nothing), and `held`, the same stream with the camera at rest (every frame from the fifth on reuses it).
Each series: 200 ms of untimed frames, then `frames` frames queued back to back and one wait; best and median of `repeats`.
python tools/classify_reuse_rate.py [frames] [repeats]   (GPU box; FT_OPTS="classify_reuse=0,..." sets options).  Prints one JSON line."""
import json, math, os, statistics, sys, time
import ctypes as C
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from functracer_amd import _capi


def orbit(cam, k, step_deg=0.05):
    """The eye circles the point it looks at about the y axis."""
    o, look = np.array(cam.o[:]), np.array(cam.look_at[:])
    a, v = math.radians(k * step_deg), o - look
    out = _capi.ft_camera.from_buffer_copy(cam)
    out.o = (C.c_double * 3)(look[0] + math.cos(a) * v[0] + math.sin(a) * v[2], look[1] + v[1], look[2] - math.sin(a) * v[0] + math.cos(a) * v[2])
    return out


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wl = ft.parse_scene_file(os.path.join(root, "scenes", "bunny.scene"))
    res_h, res_v, spp = 1920, 1080, 16
    jit = ft.jitter_pattern(spp)
    ctx = ft.Context(0)
    for kv in filter(None, os.environ.get("FT_OPTS", "").split(",")):
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    wl.lower(ctx)
    cams = [orbit(wl.camera, k) for k in range(frames)]
    counts = getattr(ctx, "classify_reuse", None)                   # (a library from before the option has no such export)
    out = {"res": [res_h, res_v], "spp": spp, "frames": frames, "repeats": repeats, "options": os.environ.get("FT_OPTS", "")}
    for series in ("orbit", "held"):
        cam_of = (lambda k: cams[k]) if series == "orbit" else (lambda k: wl.camera)
        t_end = time.perf_counter() + 0.2
        k = 0
        while time.perf_counter() < t_end:                          # clock ramp, as bench.py's --prewarm-ms
            ctx.render_enqueue(cam_of(k % frames), res_h, res_v, spp, jit)
            k += 1
        ctx.wait()
        before = counts() if counts else None
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for k in range(frames):
                ctx.render_enqueue(cam_of(k), res_h, res_v, spp, jit)
            ctx.wait()
            ms.append((time.perf_counter() - t0) * 1e3 / frames)
        out[series] = {"ms_per_frame_best": round(min(ms), 4), "ms_per_frame_median": round(statistics.median(ms), 4), "ms_per_frame_all": [round(v, 4) for v in ms]}
        if counts:
            now = counts()
            out[series]["classify_reuse"] = {k: now[k] - before[k] for k in now}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

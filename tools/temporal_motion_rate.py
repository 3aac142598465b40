#!/usr/bin/env python3
"""ft_temporal_accumulate on a scene whose objects move (ft_sg_set_transform + ft_scene_commit_moved), at 1920x1080 with 1-spp frames left
in HBM, camera on temporal_rate.py's orbit.  On night-house three series of `frames` calls each, interleaved call by call so that they see
the same clocks: "static" (no commit between the calls: k_temporal<false>), "same pose" (an ft_scene_commit_moved that changes nothing
before every call: k_temporal<true>, no leaf moved) and "moving" (the crown of the tree slides 0.05 per call: k_temporal<true>, its
pixels taken back through their record).  Per series the median k_temporal time (the call's kernel time minus its guide pass), and for
the moving one the share of tile pixels on the moved leaf.  Then the ft_get_commit_times of an ft_scene_commit_moved on bunny and on
night-house (a full commit: flatten, device BVH builds, uploads), medians of `frames`.  Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import ctypes as C
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from functracer_amd import _capi
from temporal_rate import orbit


class Recorder:
    """A builder for ParsedScene.lower that hands every call to `ctx` and notes the handle and the list of each transform node."""

    def __init__(self, ctx):
        self._ctx, self.last_error, self.transforms = ctx._ctx, ctx.last_error, []
        self.table = _capi.fth_builder()
        for name, _, _ in _capi.BUILDER_SIGNATURES:
            setattr(self.table, name, getattr(ctx.table, name))
        real = ctx._lib.ft_sg_transform

        def hook(c, ts, n, child):
            handle = real(c, ts, n, child)
            self.transforms.append((handle, [(ts[i].kind, tuple(ts[i].v), ts[i].angle) for i in range(n)]))
            return handle
        self._hook = type(self.table.sg_transform)(hook)
        self.table.sg_transform = self._hook


def ops_of(recorded):
    return [(("translate", "scale", "rotate")[k], v, a) if k == _capi.ROTATE else (("translate", "scale", "rotate")[k], v) for k, v, a in recorded]


def load(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wl = ft.parse_scene_file(os.path.join(root, "scenes", name + ".scene"))
    ctx = ft.Context(0)
    rec = Recorder(ctx)
    wl.lower(rec)
    return wl, ctx, rec


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    res_h, res_v = 1920, 1080
    jit = np.zeros((1, 2))
    out = {"res": [res_h, res_v], "frames": frames}
    # the three series on night-house, one context each, interleaved
    series = {}
    for kind in ("static", "same_pose", "moving"):
        wl, ctx, rec = load("night-house")
        crown = [h for h, ops in rec.transforms if ops == [(_capi.TRANSLATE, (0.0, 7.0, 0.0), 0.0)]]
        assert len(crown) == 1, rec.transforms
        ctx.temporal_begin(res_h, res_v)
        series[kind] = dict(wl=wl, ctx=ctx, crown=crown[0], ms=[], aov=[], history=[], moved_px=0)
    for k in range(frames + 2):
        for kind, s in series.items():
            ctx, cam = s["ctx"], orbit(s["wl"].camera, k)
            if k > 0 and kind != "static":
                if kind == "moving":
                    ctx.set_transform(s["crown"], [("translate", (0.05 * k, 7.0, 0.0))])
                ctx.commit_moved()
            ctx.render(cam, res_h, res_v, 1, jit, seed=k, fetch=False)
            _, ts = ctx.temporal_accumulate(cam, 1, jit, seed=k, to_frame=1, fetch=False)
            if k >= 2:
                s["ms"].append(ts["kernel_ms"] - ts["trace_kernel_ms"]); s["aov"].append(ts["trace_kernel_ms"])
                s["history"].append(ctx.temporal_status()["with_history"])
    s = series["moving"]
    m2w, _ = s["ctx"].leaf_matrices()
    leaf = int(np.argmin(np.abs(m2w[:, :, 3] - np.array([-8.0 + 0.05 * (frames + 1), 7.0, -5.0])).sum(-1)))
    seen = s["ctx"].render_aov(orbit(s["wl"].camera, frames + 1), res_h, res_v, 1, jit, seed=frames + 1, channels=["leaf"])["leaf"]
    out["night-house"] = {kind: {"k_temporal_ms": round(statistics.median(v["ms"]), 4), "k_temporal_ms_min_max": [round(min(v["ms"]), 4), round(max(v["ms"]), 4)],
                                 "k_aov_ms": round(statistics.median(v["aov"]), 3), "pixels_with_history": int(statistics.median(v["history"]))}
                          for kind, v in series.items()}
    out["night-house"]["share_of_pixels_on_the_moved_leaf"] = round(float((seen == leaf).mean()), 4)
    for v in series.values():
        v["ctx"].temporal_end(); v["ctx"].close()
    # what a commit_moved costs
    out["commit_moved_ms"] = {}
    for name in ("bunny", "night-house"):
        wl, ctx, rec = load(name)
        handle, ops = rec.transforms[0]
        times = []
        for k in range(frames):
            ctx.set_transform(handle, ops_of(ops))
            ctx.commit_moved()
            times.append(ctx.commit_times())
        out["commit_moved_ms"][name] = {key: round(statistics.median(t[key] for t in times), 3) for key in ("flatten_ms", "device_bvh_ms", "upload_ms")}
        out["commit_moved_ms"][name]["leaves"] = ctx.scene_info()["leaves"]
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

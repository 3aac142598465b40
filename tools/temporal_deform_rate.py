#!/usr/bin/env python3
"""ft_temporal_accumulate on a mesh that deforms between the calls ("temporal_follow_deformed"), at 1920x1080 with 1-spp
frames left in HBM: the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces: above the device builder's threshold) as `bspMesh 0`,
every vertex moved by refit_rate.py's twist before every call (ft_sg_set_mesh_triangles + ft_scene_commit_deformed), camera standing.
Two series of `frames` calls each, one context each, interleaved call by call so that they see the same clocks: "follow" (the option 1:
the commit snapshots the mesh's records, k_temporal<true, true> takes every mesh pixel back through its triangle) and "plain" (the option
0: k_temporal<false>, what the library did before the option existed).  Per series the median k_temporal time (the call's kernel time minus
its guide pass), the guide pass, the pixels with valid history, and the ft_get_commit_times of the ft_scene_commit_deformed before the call
(the snapshot's copy falls into upload_ms).  A library that does not know the option (FT_HIP_LIB pointing at an older build) runs the
"plain" series alone: alternate such runs with runs of this build to compare the two at option 0.
Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from refit_rate import ROOT, build, twisted


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    res_h, res_v = 1920, 1080
    jit = np.zeros((1, 2))
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    p = tris.reshape(-1, 3) * 8.0
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
    series = {}
    for kind, option in (("follow", 1), ("plain", 0)):
        ctx = ft.Context(0)
        try:
            ctx.set_option("temporal_follow_deformed", option)
        except ft.FtError:                                           # an older library: it has the plain series only
            ctx.close()
            continue
        series[kind] = dict(ctx=ctx, mesh=build(ctx, tris), k_temporal=[], k_aov=[], history=[], commit={k: [] for k in ("flatten_ms", "device_bvh_ms", "upload_ms")})
        ctx.temporal_begin(res_h, res_v)
    if not series:
        ctx = ft.Context(0)
        series["plain"] = dict(ctx=ctx, mesh=build(ctx, tris), k_temporal=[], k_aov=[], history=[], commit={k: [] for k in ("flatten_ms", "device_bvh_ms", "upload_ms")})
        ctx.temporal_begin(res_h, res_v)
    for k in range(frames + 2):
        shape = twisted(tris, k)
        for s in series.values():
            ctx = s["ctx"]
            if k > 0:
                ctx.set_mesh_triangles(s["mesh"], shape)
                ctx.commit_deformed()
                t = ctx.commit_times()
            ctx.render(cam, res_h, res_v, 1, jit, seed=k, fetch=False)
            _, ts = ctx.temporal_accumulate(cam, 1, jit, seed=k, fetch=False)
            if k >= 2:
                s["k_temporal"].append(ts["kernel_ms"] - ts["trace_kernel_ms"]); s["k_aov"].append(ts["trace_kernel_ms"])
                s["history"].append(ctx.temporal_status()["with_history"])
                for key in s["commit"]:
                    s["commit"][key].append(t[key])
    out = {"res": [res_h, res_v], "frames": frames, "faces": int(tris.shape[0]), "library": "FT_HIP_LIB" if os.environ.get("FT_HIP_LIB") else "this build"}
    for kind, s in series.items():
        out[kind] = {"k_temporal_ms": stats(s["k_temporal"]), "k_aov_ms": stats(s["k_aov"]), "pixels_with_history": int(statistics.median(s["history"])),
                     "commit_deformed_ms": {key: stats(v) for key, v in s["commit"].items()}}
        s["ctx"].temporal_end(); s["ctx"].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

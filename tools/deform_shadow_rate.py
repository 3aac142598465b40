#!/usr/bin/env python3
"""What "deform_light_space" is worth and what it costs, on the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as
`bspMesh 0` under one directional light, 1920 x 1080 x 16.
Tree quality: k_primary time after 1, 4 and 16 accumulated steps (or the steps of the second argument, "1,4,8,12,16") of tools/refit_rate.py's twist (0.05 rad per step between the mesh's
bottom and top; one ft_scene_commit_deformed per step), measured three ways in one process, a frame of each in turn, `frames` times:
after ft_scene_commit_deformed with the option at 1 (the full commit's light-space tree refit, the grid built again), after
ft_scene_commit_deformed with the option at 0 (the pairs stripped: the shadow rays walk the refit BVH) and after a full ft_scene_commit
of the same vertices.  Medians with min and max, the two ratios, and whether the three frames are identical.
Commit cost, measured first with no frame in flight: ft_get_commit_times of sixteen steps' ft_scene_commit_deformed with the option at 0
and at 1, alternated, and of a full commit of every fourth step's vertices; medians with min and max, and every total.
Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from refit_rate import twisted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 16
KEYS = ("flatten_ms", "device_bvh_ms", "upload_ms")


def build(ctx, tris):
    ctx.clear()
    m = ctx.bsp_mesh(0, tris)
    ctx.set_objects(ctx.group([ctx.material(ctx.scale((8.0, 8.0, 8.0), m), colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    ctx.add_directional((-3, -2, 3), (1, 1, 1))
    ctx.commit()
    return m


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def note(cost, ctx):
    t = ctx.commit_times()
    for k in KEYS:
        cost[k].append(t[k])
    cost["total_ms"].append(sum(t[k] for k in KEYS))


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    measured = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 4, 16]
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    p = tris.reshape(-1, 3) * 8.0
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
    jit = ft.jitter_pattern(SPP)
    names = ("option_1", "option_0", "full_commit")
    ctxs = {k: ft.Context(0) for k in names}
    ctxs["option_1"].set_option("deform_light_space", 1)
    cost = {k: {key: [] for key in KEYS + ("total_ms",)} for k in names}
    # commit cost first, with nothing in flight: a commit waits for the frames its context still has queued, and an upload from pageable
    # memory for every stream of the process, so a commit timed between asynchronous frames is timed with their tails
    mesh = {k: build(ctxs[k], tris) for k in ("option_1", "option_0")}
    for step in range(1, 17):
        moved = twisted(tris, step)
        for k in ("option_1", "option_0"):
            ctxs[k].set_mesh_triangles(mesh[k], moved)
            ctxs[k].commit_deformed()
            note(cost[k], ctxs[k])
        if step % 4 == 0:
            build(ctxs["full_commit"], moved)
            note(cost["full_commit"], ctxs["full_commit"])
    out = {"faces": int(tris.shape[0]), "frames": frames, "frame": [W, H, SPP], "twist_rad_per_step": 0.05, "k_primary_ms": {}}
    out["commit_cost_ms"] = {k: dict({key: stats(v) for key, v in c.items()}, commits=len(c["total_ms"])) for k, c in cost.items()}
    out["commit_total_ms_each"] = {k: [round(x, 3) for x in c["total_ms"]] for k, c in cost.items()}
    # tree quality, from the rest pose again
    mesh = {k: build(ctxs[k], tris) for k in ("option_1", "option_0")}
    for step in range(1, max(measured) + 1):
        moved = twisted(tris, step)
        for k in ("option_1", "option_0"):
            ctxs[k].set_mesh_triangles(mesh[k], moved)
            ctxs[k].commit_deformed()
        if step not in measured:
            continue
        build(ctxs["full_commit"], moved)
        ms = {k: [] for k in names}
        for r in range(frames + 2):                                 # a frame of each in turn; the first two rounds warm up
            for k in names:
                ctxs[k].render(cam, W, H, SPP, jit, fetch=False)
                if r >= 2:
                    ms[k].append(ctxs[k].kernel_times()["primary"]["ms"])
        small = [ctxs[k].render(cam, 480, 270, 1, np.zeros((1, 2)))[0] for k in names]
        res = {k + "_k_primary_ms": stats(ms[k]) for k in names}
        res["option_1_to_full_commit"] = round(res["option_1_k_primary_ms"]["median"] / res["full_commit_k_primary_ms"]["median"], 3)
        res["option_1_to_option_0"] = round(res["option_1_k_primary_ms"]["median"] / res["option_0_k_primary_ms"]["median"], 3)
        res["frames_identical"] = bool(np.array_equal(small[0], small[1]) and np.array_equal(small[0], small[2]))
        out["k_primary_ms"][str(step)] = res
    for c in ctxs.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

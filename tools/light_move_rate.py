#!/usr/bin/env python3
"""What ft_scene_commit_lights costs and what the refit light-space tree is worth, on the full-size stand-in mesh (bunny_synth_full.ply,
69.6 K faces) as `bspMesh 0` under one directional light, 1920 x 1080 x 16.
Commit cost: ft_get_commit_times of an ft_scene_commit_lights against a full ft_scene_commit of the same scene with the new direction, in
the same process, `rounds` of each, alternating; medians with min and max.  With --tree PATH the package is imported from another
checkout (the parent commit's, which has no setters) and only the full commit is measured: the graph built again with the new direction.
Tree quality: k_primary time after the light has turned by 1, 10, 45, 90 and 180 degrees about the vertical axis from the direction the
scene was committed with - after ft_scene_commit_lights (the committed direction's tree refit, the grid built again), after a full commit
at that direction, and with "light_space_shadows" = 0 at that direction; medians of `frames` frames, and whether the frames are identical.
Prints one JSON line; run on the GPU box."""
import argparse, json, math, os, statistics, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("rounds", nargs="?", type=int, default=7)
ap.add_argument("frames", nargs="?", type=int, default=7)
ap.add_argument("--tree", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
import functracer_amd as ft

W, H, SPP = 1920, 1080, 16
DIR0 = np.array([-3.0, -2.0, 3.0])
KEYS = ("flatten_ms", "device_bvh_ms", "upload_ms")


def turned(deg):
    a = math.radians(deg)
    return (math.cos(a) * DIR0[0] + math.sin(a) * DIR0[2], DIR0[1], -math.sin(a) * DIR0[0] + math.cos(a) * DIR0[2])


def build(ctx, tris, direction):
    ctx.clear()
    m = ctx.bsp_mesh(0, tris)
    ctx.set_objects(ctx.group([ctx.material(ctx.scale((8.0, 8.0, 8.0), m), colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    ctx.add_directional(direction, (1, 1, 1))
    ctx.commit()


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def primary_ms(ctx, cam, jit, frames):
    ms = []
    for k in range(frames + 2):
        ctx.render(cam, W, H, SPP, jit, fetch=False)
        if k >= 2:
            ms.append(ctx.kernel_times()["primary"]["ms"])
    return stats(ms)


def main():
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    p = tris.reshape(-1, 3) * 8.0
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
    jit = ft.jitter_pattern(SPP)
    out = {"faces": int(tris.shape[0]), "rounds": args.rounds, "frames": args.frames, "frame": [W, H, SPP], "build": "another checkout (--tree)" if args.tree else "this checkout"}
    ctx = ft.Context(0)
    hows = ("commit",) if args.tree else ("commit_lights", "commit")
    cost = {how: {k: [] for k in KEYS + ("total_ms",)} for how in hows}
    build(ctx, tris, tuple(DIR0))
    for r in range(args.rounds):
        for how in hows:
            d = turned(3.0 * (2 * r + 1 + (how == "commit")))
            if how == "commit_lights":
                ctx.set_directional(0, d, (1, 1, 1))
                ctx.commit_lights()
            else:
                build(ctx, tris, d)
            t = ctx.commit_times()
            for k in KEYS:
                cost[how][k].append(t[k])
            cost[how]["total_ms"].append(sum(t[k] for k in KEYS))
    out["commit_cost_ms"] = {how: {k: stats(v) for k, v in c.items()} for how, c in cost.items()}
    if not args.tree:
        fresh, plain = ft.Context(0), ft.Context(0)
        plain.set_option("light_space_shadows", 0)
        out["tree_quality"] = {}
        for deg in (1, 10, 45, 90, 180):
            build(ctx, tris, tuple(DIR0))
            ctx.set_directional(0, turned(deg), (1, 1, 1))
            ctx.commit_lights()
            build(fresh, tris, turned(deg))
            build(plain, tris, turned(deg))
            a, b, c = (primary_ms(x, cam, jit, args.frames) for x in (ctx, fresh, plain))
            small = [x.render(cam, 480, 270, 1, np.zeros((1, 2)))[0] for x in (ctx, fresh, plain)]
            out["tree_quality"][str(deg)] = {"commit_lights_k_primary_ms": a, "full_commit_k_primary_ms": b, "option_0_k_primary_ms": c,
                                             "to_full_commit": round(a["median"] / b["median"], 3), "to_option_0": round(a["median"] / c["median"], 3),
                                             "frames_identical": bool(np.array_equal(small[0], small[1]) and np.array_equal(small[0], small[2]))}
        fresh.close(), plain.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

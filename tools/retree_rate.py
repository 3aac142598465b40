#!/usr/bin/env python3
"""What "light_space_retree" is worth and what it costs, on the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as
`bspMesh 0` under one directional light, 1920 x 1080 x 16 (tools/light_move_rate.py's scene and turns, tools/deform_shadow_rate.py's twist).
Four ways, each a context of its own in one process, a frame of each in turn, `frames` times after two rounds that warm up:
  retree       the option at 1: the code under test
  refit        the option at 0: the full commit's topology boxed again - the behaviour before the option
  full_commit  a fresh ft_scene_commit of the same scene: the reference
  bvh          "light_space_shadows" 0 in a fresh commit: the shadow rays walk the BVH
Turns: k_primary after the light has turned by 1, 10, 45, 90 and 180 degrees about the vertical from the committed direction, one
ft_scene_commit_lights from the committed state.  Twist: after 1, 4, 8 and 16 accumulated steps of 0.05 rad, one
ft_scene_commit_deformed per step under "deform_light_space" 1.  Medians with min and max, and whether the four small frames are identical.
Commit cost: ft_get_commit_times of ft_scene_commit_lights (turns of 3 degrees) with and without the option and of the full commit,
alternated, `rounds` each; the same for sixteen twist steps' ft_scene_commit_deformed.
Prints one JSON line; run on the GPU box."""
import json, math, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from refit_rate import twisted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 16
DIR0 = np.array([-3.0, -2.0, 3.0])
KEYS = ("flatten_ms", "device_bvh_ms", "upload_ms")
WAYS = ("retree", "refit", "full_commit", "bvh")


def turned(deg):
    a = math.radians(deg)
    return (math.cos(a) * DIR0[0] + math.sin(a) * DIR0[2], DIR0[1], -math.sin(a) * DIR0[0] + math.cos(a) * DIR0[2])


def build(ctx, tris, direction):
    ctx.clear()
    m = ctx.bsp_mesh(0, tris)
    ctx.set_objects(ctx.group([ctx.material(ctx.scale((8.0, 8.0, 8.0), m), colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    ctx.add_directional(direction, (1, 1, 1))
    ctx.commit()
    return m


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def note(cost, ctx):
    t = ctx.commit_times()
    for k in KEYS:
        cost[k].append(t[k])
    cost["total_ms"].append(sum(t[k] for k in KEYS))


def frames_of(ctxs, cam, jit, frames):
    ms = {k: [] for k in WAYS}
    for r in range(frames + 2):                                     # a frame of each in turn; the first two rounds warm up
        for k in WAYS:
            ctxs[k].render(cam, W, H, SPP, jit, fetch=False)
            if r >= 2:
                ms[k].append(ctxs[k].kernel_times()["primary"]["ms"])
    small = [ctxs[k].render(cam, 480, 270, 1, np.zeros((1, 2)))[0] for k in WAYS]
    res = {k + "_k_primary_ms": stats(ms[k]) for k in WAYS}
    med = {k: res[k + "_k_primary_ms"]["median"] for k in WAYS}
    res["retree_to_full_commit"] = round(med["retree"] / med["full_commit"], 3)
    res["refit_to_full_commit"] = round(med["refit"] / med["full_commit"], 3)
    res["retree_to_bvh"] = round(med["retree"] / med["bvh"], 3)
    res["frames_identical"] = bool(all(np.array_equal(small[0], s) for s in small[1:]))
    return res


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    p = tris.reshape(-1, 3) * 8.0
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
    jit = ft.jitter_pattern(SPP)
    ctxs = {k: ft.Context(0) for k in WAYS}
    ctxs["retree"].set_option("light_space_retree", 1)
    ctxs["bvh"].set_option("light_space_shadows", 0)
    for k in ("retree", "refit"):
        ctxs[k].set_option("deform_light_space", 1)
    out = {"faces": int(tris.shape[0]), "rounds": rounds, "frames": frames, "frame": [W, H, SPP]}
    # commit cost first, with no frame in flight
    hows = ("retree", "refit", "full_commit")
    cost = {k: {key: [] for key in KEYS + ("total_ms",)} for k in hows}
    for k in ("retree", "refit"):
        build(ctxs[k], tris, tuple(DIR0))
    for r in range(rounds):
        for n, k in enumerate(hows):
            d = turned(3.0 * (3 * r + 1 + n))
            if k == "full_commit":
                build(ctxs[k], tris, d)
            else:
                ctxs[k].set_directional(0, d, (1, 1, 1))
                ctxs[k].commit_lights()
            note(cost[k], ctxs[k])
    out["commit_lights_cost_ms"] = {k: {key: stats(v) for key, v in c.items()} for k, c in cost.items()}
    cost = {k: {key: [] for key in KEYS + ("total_ms",)} for k in hows}
    mesh = {k: build(ctxs[k], tris, tuple(DIR0)) for k in ("retree", "refit")}
    for step in range(1, 17):
        moved = twisted(tris, step)
        for k in ("retree", "refit"):
            ctxs[k].set_mesh_triangles(mesh[k], moved)
            ctxs[k].commit_deformed()
            note(cost[k], ctxs[k])
        if step % 4 == 0:
            build(ctxs["full_commit"], moved, tuple(DIR0))
            note(cost["full_commit"], ctxs["full_commit"])
    out["commit_deformed_cost_ms"] = {k: dict({key: stats(v) for key, v in c.items()}, commits=len(c["total_ms"])) for k, c in cost.items()}
    # k_primary after a turn
    out["turn_k_primary_ms"] = {}
    for deg in (1, 10, 45, 90, 180):
        for k in ("retree", "refit"):
            build(ctxs[k], tris, tuple(DIR0))
            ctxs[k].set_directional(0, turned(deg), (1, 1, 1))
            ctxs[k].commit_lights()
        for k in ("full_commit", "bvh"):
            build(ctxs[k], tris, turned(deg))
        out["turn_k_primary_ms"][str(deg)] = frames_of(ctxs, cam, jit, frames)
    # k_primary along the twist, from the rest pose again
    out["twist_k_primary_ms"] = {}
    mesh = {k: build(ctxs[k], tris, tuple(DIR0)) for k in ("retree", "refit")}
    for step in range(1, 17):
        moved = twisted(tris, step)
        for k in ("retree", "refit"):
            ctxs[k].set_mesh_triangles(mesh[k], moved)
            ctxs[k].commit_deformed()
        if step not in (1, 4, 8, 16):
            continue
        for k in ("full_commit", "bvh"):
            build(ctxs[k], moved, tuple(DIR0))
        out["twist_k_primary_ms"][str(step)] = frames_of(ctxs, cam, jit, frames)
    for c in ctxs.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What "moved_in_place" saves and what it costs, on the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as `bspMesh 0`
under a transform node and one directional light, 1920 x 1080 x 16 (tools/retree_rate.py's scene and view).  The mesh turns about the
vertical through the middle of its bounds.  Four ways, each a context of its own in one process:
  off          the option at 0: ft_scene_commit_moved is the full commit - the behaviour before the option
  in_place     the option at 1, "light_space_retree" 0: the poses uploaded, the pair's tree refit, its grid built again
  retree       the option at 1, "light_space_retree" 1: the tree's topology built again as well
  fresh        a new ft_scene_commit of a graph built at the pose: the reference
Moves: a translation; turns of 1, 10, 45 and 90 degrees from the full-commit pose; sixteen steps of 5 degrees.  Per move and way
ft_get_commit_times of the call (`rounds` calls; each turn from a full commit at the rest pose, which the first call after a full commit
pays its tables for; the translations and the steps follow one another) and k_primary's time on the frames that follow (`frames` frames
of each way in turn after two rounds that warm up) - medians with min and max - and whether the four ways' small frames are identical.
A library that does not know the option (FT_HIP_LIB pointing at an older build) runs the `off` and `fresh` series alone: the baseline for
what the call cost before.
Prints one JSON line; run on the GPU box."""
import json, math, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 16
DIR0 = (-3.0, -2.0, 3.0)
KEYS = ("flatten_ms", "device_bvh_ms", "upload_ms")
TURNS = (1, 10, 45, 90)


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    p = tris.reshape(-1, 3) * 8.0
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
    jit = ft.jitter_pattern(SPP)

    def pose(deg=0.0, shift=(0.0, 0.0, 0.0)):
        c = tuple(float(x) for x in centre)
        return [("scale", (8.0, 8.0, 8.0)), ("translate", tuple(-x for x in c)), ("rotate", (0, 1, 0), math.radians(deg)),
                ("translate", tuple(x + s for x, s in zip(c, shift)))]

    def build(ctx, ops):
        ctx.clear()
        node = ctx.transform(ops, ctx.bsp_mesh(0, tris))
        ctx.set_objects(ctx.group([ctx.material(node, colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
        ctx.add_directional(DIR0, (1, 1, 1))
        ctx.commit()
        return node

    ctxs = {k: ft.Context(0) for k in ("off", "in_place", "retree", "fresh")}
    ways = ["off"]
    try:
        for k in ("in_place", "retree"):
            ctxs[k].set_option("moved_in_place", 1)
        ctxs["retree"].set_option("light_space_retree", 1)
        ways += ["in_place", "retree"]
    except ft.FtError:
        pass                                                        # an older library: the baseline series alone
    out = {"faces": int(tris.shape[0]), "rounds": rounds, "frames": frames, "frame": [W, H, SPP], "ways": ways,
           "library": "FT_HIP_LIB" if os.environ.get("FT_HIP_LIB") else "this build"}

    def new_cost():
        return {k: {key: [] for key in KEYS + ("total_ms",)} for k in ways + ["fresh"]}

    def note(cost, k):
        t = ctxs[k].commit_times()
        for key in KEYS:
            cost[k][key].append(t[key])
        cost[k]["total_ms"].append(sum(t[key] for key in KEYS))

    def move(k, node, ops):
        ctxs[k].set_transform(node, ops)
        ctxs[k].commit_moved()

    def frames_of(kinds):
        ms = {k: [] for k in kinds}
        for r in range(frames + 2):                                 # a frame of each in turn; the first two rounds warm up
            for k in kinds:
                ctxs[k].render(cam, W, H, SPP, jit, fetch=False)
                if r >= 2:
                    ms[k].append(ctxs[k].kernel_times()["primary"]["ms"])
        small = [ctxs[k].render(cam, 480, 270, 1, np.zeros((1, 2)))[0] for k in kinds]
        res = {k: stats(ms[k]) for k in kinds}
        res["frames_identical"] = bool(all(np.array_equal(small[0], s, equal_nan=True) for s in small[1:]))
        return res

    def summary(cost):
        return {k: {key: stats(v) for key, v in c.items()} for k, c in cost.items() if c["total_ms"]}

    # a translation: `rounds` of them, one after the other
    node = {k: build(ctxs[k], pose()) for k in ways}
    cost = new_cost()
    for r in range(rounds):
        ops = pose(0.0, (0.01 * (r + 1), 0.0, -0.005 * (r + 1)))
        for k in ways:
            move(k, node[k], ops)
            note(cost, k)
        build(ctxs["fresh"], ops)
        note(cost, "fresh")
    out["translation"] = {"commit_ms": summary(cost), "k_primary_ms": frames_of(ways + ["fresh"])}
    # turns from the full-commit pose
    out["turn"] = {}
    for deg in TURNS:
        cost = new_cost()
        for r in range(rounds):
            for k in ways:
                node[k] = build(ctxs[k], pose())
                move(k, node[k], pose(deg))
                note(cost, k)
            build(ctxs["fresh"], pose(deg))
            note(cost, "fresh")
        out["turn"][str(deg)] = {"commit_ms": summary(cost), "k_primary_ms": frames_of(ways + ["fresh"])}
    # sixteen steps of 5 degrees
    node = {k: build(ctxs[k], pose()) for k in ways}
    cost = new_cost()
    for step in range(1, 17):
        for k in ways:
            move(k, node[k], pose(5.0 * step))
            note(cost, k)
        build(ctxs["fresh"], pose(5.0 * step))
        note(cost, "fresh")
    out["steps_of_5"] = {"commit_ms": summary(cost), "k_primary_ms_after_16": frames_of(ways + ["fresh"])}
    if "in_place" in ways:
        out["moved_commits"] = {k: ctxs[k].moved_commits() for k in ways}
    for c in ctxs.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What ft_scene_commit_deformed costs and what the refit tree is worth, on the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K
faces) as `bspMesh 0` under "bvh_builder" 0 and 3.
Commit cost: ft_get_commit_times of an ft_scene_commit_deformed against an ft_scene_commit of the same edited graph in the same process
(the parent's path), `rounds` of each, alternating; medians with min and max.  Where the tree can be rebuilt in place (builder 3), also
`rounds` of an ft_scene_commit_deformed that rebuilds ("refit_rebuild_percent" = 200 and, each round, another permutation of the
triangles - the worst case for a tree that keeps its topology), with how many of them did rebuild.
Tree quality: k_primary time of a 1920x1080, 1-spp frame after 1, 4 and 16 accumulated steps of a twist about the vertical axis (0.05 rad
per step between the mesh's bottom and top), traced on the refit tree (one refit per step, each of the previous refit's tree) and on a
freshly built tree of the same vertices; medians of `frames` frames.  Beside each k_primary ratio stands the cost ratio
ft_scene_tree_quality measures for the refit tree (cost now / cost as built), which is what a host sets "refit_rebuild_percent" by.
Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 0.05


def twisted(tris, steps):
    p = tris.reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    c = 0.5 * (lo + hi)
    ang = STEP * steps * (p[:, 1] - lo[1]) / (hi[1] - lo[1])
    x, z = p[:, 0] - c[0], p[:, 2] - c[2]
    out = np.stack([c[0] + np.cos(ang) * x + np.sin(ang) * z, p[:, 1], c[2] - np.sin(ang) * x + np.cos(ang) * z], axis=1)
    return np.ascontiguousarray(out.reshape(-1, 9))


def build(ctx, tris):
    ctx.clear()
    m = ctx.bsp_mesh(0, tris)
    ctx.set_objects(ctx.group([ctx.material(ctx.scale((8.0, 8.0, 8.0), m), colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    ctx.add_directional((-3, -2, 3), (1, 1, 1))
    ctx.commit()
    return m


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def primary_ms(ctx, cam, frames):
    jit = np.zeros((1, 2))
    ms = []
    for k in range(frames + 2):
        ctx.render(cam, 1920, 1080, 1, jit, fetch=False)
        if k >= 2:
            ms.append(ctx.kernel_times()["primary"]["ms"])
    return stats(ms)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    p = tris.reshape(-1, 3) * 8.0
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
    out = {"faces": int(tris.shape[0]), "rounds": rounds, "frames": frames, "twist_rad_per_step": STEP, "builders": {}}
    for builder in (0, 3):
        ctx = ft.Context(0)
        ctx.set_option("bvh_builder", builder)
        m = build(ctx, tris)
        keys = ("flatten_ms", "device_bvh_ms", "upload_ms")
        cost = {"commit_deformed": {k: [] for k in keys + ("total_ms",)}, "commit": {k: [] for k in keys + ("total_ms",)}}
        first = None
        for r in range(rounds):
            for how in ("commit_deformed", "commit"):
                ctx.set_mesh_triangles(m, twisted(tris, 0.1 * (r + 1)))
                getattr(ctx, how)()
                t = ctx.commit_times()
                if how == "commit_deformed" and first is None:
                    first = {k: round(t[k], 3) for k in keys}     # the first refit after a full commit also derives the parent links
                for k in keys:
                    cost[how][k].append(t[k])
                cost[how]["total_ms"].append(sum(t[k] for k in keys))
        res = {"commit_cost_ms": {how: {k: stats(v) for k, v in c.items()} for how, c in cost.items()}, "first_refit_ms": first, "tree_quality": {}}
        if ctx.tree_quality(m)["rebuildable"]:                       # a commit that rebuilds in place
            build(ctx, tris)
            ctx.set_option("refit_rebuild_percent", 200)
            c, rebuilt = {k: [] for k in keys + ("total_ms",)}, 0
            for r in range(rounds):
                before = ctx.tree_quality(m)["rebuilds"]
                ctx.set_mesh_triangles(m, tris[np.random.default_rng(r).permutation(tris.shape[0])])
                ctx.commit_deformed()
                t = ctx.commit_times()
                rebuilt += ctx.tree_quality(m)["rebuilds"] - before
                for k in keys:
                    c[k].append(t[k])
                c["total_ms"].append(sum(t[k] for k in keys))
            res["commit_cost_ms"]["commit_deformed_rebuild"] = dict({k: stats(v) for k, v in c.items()}, rebuilt=rebuilt)
            ctx.set_option("refit_rebuild_percent", 0)
        # tree quality: refit step by step from the rest pose, against a fresh build of the same vertices
        build(ctx, tris)
        fresh = ft.Context(0)
        fresh.set_option("bvh_builder", builder)
        res["tree_quality"]["0"] = {"fresh_k_primary_ms": primary_ms(ctx, cam, frames), "cost": round(ctx.tree_quality(m)["cost"], 4)}
        for step in range(1, 17):
            ctx.set_mesh_triangles(m, twisted(tris, step))
            ctx.commit_deformed()
            if step in (1, 4, 16):
                a = primary_ms(ctx, cam, frames)
                build(fresh, twisted(tris, step))
                b = primary_ms(fresh, cam, frames)
                same = bool(np.array_equal(ctx.render(cam, 480, 270, 1, np.zeros((1, 2)))[0], fresh.render(cam, 480, 270, 1, np.zeros((1, 2)))[0]))
                res["tree_quality"][str(step)] = {"refit_k_primary_ms": a, "fresh_k_primary_ms": b, "ratio": round(a["median"] / b["median"], 3),
                                                  "cost_ratio": round(ctx.tree_quality(m)["ratio"], 3), "frames_identical": same}
        out["builders"][str(builder)] = res
        ctx.close(), fresh.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

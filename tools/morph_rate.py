#!/usr/bin/env python3
"""What morph targets on the device are worth, on the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as `bspMesh 0` under one
directional light, with nothing in flight.  For K = 1, 4 and 16 key shapes (tools/refit_rate.py's twist at growing angles) sixteen poses
are committed three ways, a step of each in turn, each in a context of its own in one process:
  (a) the host blends the pose in numpy (functracer_amd.morph_blend's arithmetic on deltas made once), set_mesh_triangles, commit_deformed
      - the only route there was before ft_sg_set_mesh_weights;
  (b) set_mesh_weights, commit_deformed with "morph_on_device" 0: the library's host blends;
  (c) set_mesh_weights, commit_deformed with "morph_on_device" 1: k_morph_blend and the device scan.
Per way and K: median (min - max) of ft_get_commit_times [0] host / [1] kernels / [2] uploads of the commits, and of the wall time of the
whole step { make the pose, hand it over, commit_deformed }.  The first pose of (c) uploads base and deltas and is reported apart.
(c) also runs once under "deform_light_space" 1 at K = 4, beside (a) under the same option.
Prints one JSON line; run on the GPU box."""
import json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
from refit_rate import twisted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("flatten_ms", "device_bvh_ms", "upload_ms")
POSES = 16


def build(ctx, tris):
    ctx.clear()
    m = ctx.bsp_mesh(0, tris)
    ctx.set_objects(ctx.group([ctx.material(ctx.scale((8.0, 8.0, 8.0), m), colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    ctx.add_directional((-3, -2, 3), (1, 1, 1))
    ctx.commit()
    return m


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def run(tris, k_targets, light_space, ways):
    targets = np.stack([twisted(tris, 2 * (k + 1)) for k in range(k_targets)])
    deltas = targets - tris                                         # (a)'s host keeps deltas too: its blend is the formula's loop
    ctxs, mesh = {}, {}
    for way in ways:
        ctxs[way] = ft.Context(0)
        ctxs[way].set_option("deform_light_space", light_space)
        ctxs[way].set_option("morph_on_device", 1 if way == "c" else 0)
        mesh[way] = build(ctxs[way], tris)
        if way != "a":
            ctxs[way].set_mesh_targets(mesh[way], targets)
    rows = {way: {key: [] for key in KEYS + ("step_wall_ms",)} for way in ways}
    first_c = None
    for pose in range(POSES + 1):                                   # pose 0 warms up (and uploads (c)'s base and deltas)
        w = np.array([0.5 + 0.5 * np.sin(0.4 * pose + k) for k in range(k_targets)]) / k_targets
        for way in ways:
            ctx = ctxs[way]
            t0 = time.perf_counter()
            if way == "a":
                acc = tris.copy()
                for k in range(k_targets):
                    acc = acc + w[k] * deltas[k]
                ctx.set_mesh_triangles(mesh[way], acc)
            else:
                ctx.set_mesh_weights(mesh[way], w)
            ctx.commit_deformed()
            wall = (time.perf_counter() - t0) * 1e3
            t = ctx.commit_times()
            if pose == 0:
                if way == "c":
                    first_c = dict({k: round(t[k], 3) for k in KEYS}, step_wall_ms=round(wall, 3))
                continue
            for key in KEYS:
                rows[way][key].append(t[key])
            rows[way]["step_wall_ms"].append(wall)
    same = True
    if "a" in ways and "c" in ways:
        ta, tc = ctxs["a"].mesh_trees(), ctxs["c"].mesh_trees()
        same = all(np.array_equal(ta[k].view(np.uint8), tc[k].view(np.uint8)) for k in ("tris", "wide", "coarse_boxes"))
    morph = ctxs["c"].morph(mesh["c"]) if "c" in ways else None
    for c in ctxs.values():
        c.close()
    out = {way: {key: stats(v) for key, v in r.items()} for way, r in rows.items()}
    out["c_first_pose"] = first_c
    out["a_and_c_trees_identical"] = bool(same)
    if morph:
        out["resident_bytes"] = morph["resident_bytes"]
    return out


def main():
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    out = {"faces": int(tris.shape[0]), "poses": POSES, "ways": {"a": "numpy blend + set_mesh_triangles", "b": "weights, morph_on_device 0", "c": "weights, morph_on_device 1"},
           "columns": {"flatten_ms": "[0] host", "device_bvh_ms": "[1] kernels and readbacks", "upload_ms": "[2] uploads"}, "K": {}}
    for k_targets in (1, 4, 16):
        out["K"][str(k_targets)] = run(tris, k_targets, 0, ("a", "b", "c"))
    out["deform_light_space_1_K4"] = run(tris, 4, 1, ("a", "c"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

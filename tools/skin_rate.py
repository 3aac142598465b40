#!/usr/bin/env python3
"""What skinning on the device is worth, on the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as `bspMesh 0` under one
directional light, with nothing in flight.  The mesh is skinned along its height: a corner's bones are the n_bones segments around its
y, J of them, with weights that fall off and sum to 1 (equal positions get equal influences: the mesh stays welded); a pose turns every
bone about the y axis by an angle that grows with the bone and swings with the pose.  Sixteen poses are committed three ways, a step of
each in turn, each in a context of its own in one process:
  (a) the host skins the pose in numpy (functracer_amd.skin_blend), set_mesh_triangles, commit_deformed - the only route there was
      before ft_sg_set_mesh_bones;
  (b) set_mesh_bones, commit_deformed with "skin_on_device" 0: the library's host skins;
  (c) set_mesh_bones, commit_deformed with "skin_on_device" 1: k_skin and the device scan.
Rows: J = 1 and 4 with 4, 64 and 256 bones; J = 4, 64 bones under "deform_light_space" 1; J = 4, 64 bones over morph targets, K = 4
((a) blends and skins in numpy, (b) and (c) set weights and bones; "morph_on_device" follows "skin_on_device").
Per way and row: median (min - max) of ft_get_commit_times [0] host / [1] kernels / [2] uploads of the commits, and of the wall time of
the whole step { make the pose, hand it over, commit_deformed }.  The first pose of (c) uploads the resident arrays and is reported apart.
--device-only: route (c) alone on three rows, for a kernel trace of k_skin.
--dq: the six J x bones rows for dual-quaternion palettes: the same bones and poses as unit dual quaternions, (a) skins
with functracer_amd.skin_blend_dq, (b) and (c) call set_mesh_bones_dq.  With --device-only: route (c) of both palette kinds on the three
rows, for one kernel trace of k_skin_dq beside k_skin.
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


def skin_of(tris, influences, n_bones):
    y = tris.reshape(-1, 3)[:, 1]
    t = (y - y.min()) / (y.max() - y.min()) * (n_bones - 1)
    first = np.clip(np.floor(t).astype(np.int64) - (influences - 1) // 2, 0, max(n_bones - influences, 0))
    index = np.minimum(first[:, None] + np.arange(influences)[None, :], n_bones - 1)
    weight = 1.0 / (1.0 + np.abs(index - t[:, None]))
    weight /= weight.sum(axis=1, keepdims=True)
    return index.astype(np.int32).reshape(-1, 3, influences), np.ascontiguousarray(weight.reshape(-1, 3, influences))


def palette(c, n_bones, pose):
    """The pose's bone matrices about the mesh's centre c."""
    out = np.zeros((n_bones, 3, 4))
    for b in range(n_bones):
        ang = 0.6 * np.sin(0.4 * pose) * (b + 1) / n_bones
        A = np.array([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]])
        out[b, :, :3], out[b, :, 3] = A, c - A @ c
    return out.reshape(n_bones, 12)


def palette_dq(c, n_bones, pose):
    """The same motions as unit dual quaternions: a turn about y through c is the rotation and the translation c - A c."""
    ang = np.array([0.6 * np.sin(0.4 * pose) * (b + 1) / n_bones for b in range(n_bones)])
    r = np.stack([np.cos(0.5 * ang), np.zeros(n_bones), np.sin(0.5 * ang), np.zeros(n_bones)], axis=1)
    t = np.stack([c[0] - (np.cos(ang) * c[0] + np.sin(ang) * c[2]), np.zeros(n_bones), c[2] - (-np.sin(ang) * c[0] + np.cos(ang) * c[2])], axis=1)
    return ft.dual_quaternions(r, t)


def run(tris, influences, n_bones, light_space, k_targets, ways, dq=False):
    index, weight = skin_of(tris, influences, n_bones)
    targets = np.stack([twisted(tris, 2 * (k + 1)) for k in range(k_targets)]) if k_targets else None
    deltas = targets - tris if k_targets else None
    p = tris.reshape(-1, 3)
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    ctxs, mesh = {}, {}
    for way in ways:
        ctxs[way] = ft.Context(0)
        ctxs[way].set_option("deform_light_space", light_space)
        ctxs[way].set_option("skin_on_device", 1 if way == "c" else 0)
        ctxs[way].set_option("morph_on_device", 1 if way == "c" else 0)
        mesh[way] = build(ctxs[way], tris)
        if way != "a":
            if k_targets:
                ctxs[way].set_mesh_targets(mesh[way], targets)
            ctxs[way].set_mesh_skin(mesh[way], index, weight)
    rows = {way: {key: [] for key in KEYS + ("step_wall_ms",)} for way in ways}
    first_c = None
    for pose in range(POSES + 1):                                   # pose 0 warms up (and uploads (c)'s resident arrays)
        w = np.array([0.5 + 0.5 * np.sin(0.4 * pose + k) for k in range(k_targets)]) / max(k_targets, 1)
        for way in ways:
            ctx = ctxs[way]
            t0 = time.perf_counter()
            bones = (palette_dq if dq else palette)(centre, n_bones, pose)   # (every way makes its own palette: part of the step)
            if way == "a":
                shape = tris
                if k_targets:
                    shape = tris.copy()
                    for k in range(k_targets):
                        shape = shape + w[k] * deltas[k]
                ctx.set_mesh_triangles(mesh[way], (ft.skin_blend_dq if dq else ft.skin_blend)(shape, index, weight, bones))
            else:
                if k_targets:
                    ctx.set_mesh_weights(mesh[way], w)
                (ctx.set_mesh_bones_dq if dq else ctx.set_mesh_bones)(mesh[way], bones)
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
    same = None
    if "a" in ways and "c" in ways:
        ta, tc = ctxs["a"].mesh_trees(), ctxs["c"].mesh_trees()
        same = all(np.array_equal(ta[k].view(np.uint8), tc[k].view(np.uint8)) for k in ("tris", "wide", "coarse_boxes"))
    skin = ctxs["c"].skin(mesh["c"]) if "c" in ways else None
    if skin and dq:
        skin["device_commits"] = ctxs["c"].skin_dq(mesh["c"])["device_commits"]
    for c in ctxs.values():
        c.close()
    out = {way: {key: stats(v) for key, v in r.items()} for way, r in rows.items()}
    out["c_first_pose"] = first_c
    if same is not None:
        out["a_and_c_trees_identical"] = bool(same)
    if "a" in ways and "c" in ways:                                 # the condition of DESIGN.md 16.5: (c) below (a) by more than the two spreads
        a, c = out["a"]["step_wall_ms"], out["c"]["step_wall_ms"]
        out["c_wins_by_more_than_the_spreads"] = bool(a["median"] - c["median"] > (a["max"] - a["min"]) + (c["max"] - c["min"]))
    if skin:
        out["resident_bytes"], out["device_commits"] = skin["resident_bytes"], skin["device_commits"]
    return out


def main():
    with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
        tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
    out = {"faces": int(tris.shape[0]), "poses": POSES, "library": os.path.basename(ft.HIP_LIB),
           "ways": {"a": "numpy skin + set_mesh_triangles", "b": "bones, skin_on_device 0", "c": "bones, skin_on_device 1"},
           "columns": {"flatten_ms": "[0] host", "device_bvh_ms": "[1] kernels and readbacks", "upload_ms": "[2] uploads"}, "rows": {}}
    dq = "--dq" in sys.argv
    if dq:
        out["palette"] = "dual quaternions"
        out["ways"] = {"a": "numpy skin_blend_dq + set_mesh_triangles", "b": "bones_dq, skin_on_device 0", "c": "bones_dq, skin_on_device 1"}
    if "--device-only" in sys.argv:
        for influences, n_bones in ((1, 4), (4, 64), (4, 256)):
            out["rows"][f"J{influences}_bones{n_bones}"] = run(tris, influences, n_bones, 0, 0, ("c",))
            if dq:
                out["rows"][f"J{influences}_bones{n_bones}_dq"] = run(tris, influences, n_bones, 0, 0, ("c",), dq=True)
    elif dq:
        for influences in (1, 4):
            for n_bones in (4, 64, 256):
                out["rows"][f"J{influences}_bones{n_bones}"] = run(tris, influences, n_bones, 0, 0, ("a", "b", "c"), dq=True)
    else:
        for influences in (1, 4):
            for n_bones in (4, 64, 256):
                out["rows"][f"J{influences}_bones{n_bones}"] = run(tris, influences, n_bones, 0, 0, ("a", "b", "c"))
        out["rows"]["J4_bones64_deform_light_space_1"] = run(tris, 4, 64, 1, 0, ("a", "c"))
        out["rows"]["J4_bones64_morph_K4"] = run(tris, 4, 64, 0, 4, ("a", "b", "c"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the queued deform commit (ft_scene_commit_deformed_enqueue) is worth to a host that poses a mesh every frame.
Two scenes at 1920 x 1080 x 16: the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as `bspMesh 0` under one directional
light, skinned to 64 bones along its height with 4 influences per corner; and hollow-sphere built by hand (its 25 CSG items of primitives
inside the shell, reflectance 0.4, one point light: milliseconds of tracing per frame) with a skinned tube of 1920 triangles standing in
front of the items.
`steps` steps of { ft_sg_set_mesh_bones, commit, ft_render_enqueue_into RGBA8 into a ring of page-locked frames }, the wall time of every
step, then one wait.  Three ways, each a context of its own:
  floor      no commit at all: the same frame queued every step
  blocking   ft_scene_commit_deformed: what the library could do before
  queued     ft_scene_commit_deformed_enqueue
Per way the median step with min, max and the 10th / 90th percentile, the wall time per step over the whole run with the final wait, and
what ft_debug_deform_queue counted.
The driver (no --child) runs every (scene, library) pair as a process of its own under its own time limit, `rounds` rounds, this build
and - with --parent-lib - an older library in turn (it runs floor and blocking alone there), and stops at the first failure.  It prints
one JSON line and, with --out, writes it to a file.  Run on the GPU box."""
import argparse, json, math, os, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 16
RING = 8
BONES, J = 64, 4
SCENES = ("bunny", "hollow-sphere")
CHILD_LIMIT_S = 240


def stats(v):
    s = sorted(v)
    return {"median": round(statistics.median(s), 4), "min": round(s[0], 4), "max": round(s[-1], 4),
            "p10": round(s[len(s) // 10], 4), "p90": round(s[(9 * len(s)) // 10], 4)}


def skin_along_y(tris):
    """Index and weight [n, 3, J]: a corner is shared by the J bones nearest to its height, by distance."""
    y = tris.reshape(-1, 3)[:, 1]
    f = (y - y.min()) / max(float(np.ptp(y)), 1e-300) * (BONES - 1)
    first = np.clip(np.floor(f).astype(np.int64) - 1, 0, BONES - J)
    index = first[:, None] + np.arange(J)[None, :]
    w = np.maximum(2.0 - np.abs(index - f[:, None]), 0.0)
    w /= w.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(index.astype(np.int32).reshape(-1, 3, J)), np.ascontiguousarray(w.reshape(-1, 3, J))


def palette(k, centre, amount):
    """[BONES, 12]: bone b turns about the vertical axis through `centre` by amount * (k % 50) * b / BONES."""
    out = np.zeros((BONES, 3, 4))
    for b in range(BONES):
        a = amount * (k % 50) * b / BONES
        R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        out[b, :, :3] = R
        out[b, :, 3] = centre - R @ centre
    return out.reshape(BONES, 12)


def tube(segments=32, rings=31, length=3.0, radius=0.35):
    def point(r, s):
        a = 2.0 * math.pi * s / segments
        return np.array([radius * math.cos(a), length * r / (rings - 1) - 0.5 * length, radius * math.sin(a)])
    tris = []
    for r in range(rings - 1):
        for s in range(segments):
            p00, p01, p10, p11 = point(r, s), point(r, s + 1), point(r + 1, s), point(r + 1, s + 1)
            tris += [np.concatenate([p00, p10, p11]), np.concatenate([p00, p11, p01])]
    return np.ascontiguousarray(np.array(tris))


def child(scene, steps, warm):
    import functracer_amd as ft
    jit = ft.jitter_pattern(SPP)
    if scene == "bunny":
        with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
            tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9)) * 8.0
        p = tris.reshape(-1, 3)
        centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
        cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)
        amount = 0.004

        def build(ctx):
            ctx.clear()
            node = ctx.bsp_mesh(0, tris)
            ctx.set_objects(ctx.group([ctx.material(node, colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
            ctx.add_directional((-3.0, -2.0, 3.0), (1, 1, 1))
            ctx.commit()
            return node
    else:
        cam = ft.make_camera((5.7, 5.7, -5.7), (0, 0, 4), (0, 1, 0), math.radians(60.0), 1.0)
        colours = ((1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1))
        tris = tube() + np.array([0.0, 0.0, -2.0] * 3)
        centre = np.array([0.0, 0.0, -2.0])
        amount = 0.02

        def build(ctx):
            ctx.clear()
            items = [ctx.material(ctx.subtract(ctx.scale(11.0, ctx.primitive(ft.SPHERE)), ctx.scale(10.0, ctx.primitive(ft.SPHERE))), colour=(0.4, 0.4, 0.4))]
            for row, y in enumerate((2.6, 1.3, 0.0, -1.3, -2.6)):
                for col, x in enumerate((-2.6, -1.3, 0.0, 1.3, 2.6)):
                    ball = ctx.scale(0.65, ctx.primitive(ft.SPHERE))
                    op = ctx.subtract if (row + col) % 2 == 0 else ctx.intersect
                    items.append(ctx.material(ctx.translate((x, y, 0.0), op(ctx.primitive(ft.CUBE), ball)), colour=colours[col], reflectance=0.4, shineyness=10.0))
            node = ctx.bsp_mesh(0, tris)
            items.append(ctx.material(node, colour=(0.9, 0.5, 0.2), shineyness=4.0))
            ctx.set_objects(ctx.group(items))
            ctx.add_positional((0, 0, -8), (1, 0.01, 0.02), (1, 1, 1))
            ctx.commit()
            return node

    index, weight = skin_along_y(tris)
    queued_known = hasattr(ft.hip_lib(), "ft_scene_commit_deformed_enqueue")
    ways = ["floor", "blocking"] + (["queued"] if queued_known else [])
    ring = [ft.PinnedArray((H, W, 4), np.uint8) for _ in range(RING)]
    palettes = [palette(k, centre, amount) for k in range(50)]
    out = {"scene": scene, "steps": steps, "triangles": int(tris.shape[0]), "library": "FT_HIP_LIB" if os.environ.get("FT_HIP_LIB") else "this build", "ways": {}}
    small = {}
    for way in ways:
        ctx = ft.Context(0)
        node = build(ctx)
        ctx.set_mesh_skin(node, index, weight)
        ctx.set_mesh_bones(node, palettes[0])
        ctx.commit_deformed()                                       # the first refit since the full commit: blocking either way
        commit = {"floor": None, "blocking": ctx.commit_deformed, "queued": getattr(ctx, "commit_deformed_enqueue", None)}[way]

        def step(k):
            if commit:
                ctx.set_mesh_bones(node, palettes[k % 50])
                commit()
            ctx.render_enqueue(cam, W, H, SPP, jit, rgba8=True, out=ring[k % RING].array)

        for k in range(warm):
            step(k)
        ctx.wait()
        ms = []
        t0 = time.perf_counter()
        for k in range(warm, warm + steps):
            t = time.perf_counter()
            step(k)
            ms.append((time.perf_counter() - t) * 1e3)
        ctx.wait()
        whole = (time.perf_counter() - t0) * 1e3 / steps
        out["ways"][way] = {"step_ms": stats(ms), "wall_ms_per_step": round(whole, 4)}
        if commit:
            out["ways"][way]["commit_times"] = ctx.commit_times()
        if way == "queued":
            out["ways"][way]["deform_queue"] = ctx.deform_queue()
        if commit:                                                  # the same last pose both ways: the frames must agree
            small[way] = ctx.render(cam, 480, 270, 1, np.zeros((1, 2)))[0]
        ctx.close()
    if "queued" in small:
        out["frames_identical"] = bool(np.array_equal(small["blocking"], small["queued"], equal_nan=True))
    for p in ring:
        p.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=SCENES)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="an older libfunctracer_hip.so, run in turn with this build (floor and blocking alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warm)
    runs = []
    for r in range(a.rounds):
        for scene in SCENES:
            for lib in (None, a.parent_lib) if a.parent_lib else (None,):
                env = dict(os.environ)
                env.pop("FT_HIP_LIB", None)
                if lib:
                    env["FT_HIP_LIB"] = os.path.abspath(lib)
                try:
                    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scene, "--steps", str(a.steps), "--warm", str(a.warm)],
                                         env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"failed": [scene, lib or "this build", "time limit"], "runs": runs}))
                    return 1
                if res.returncode != 0:                             # the first failure ends the run: nothing more is started on the device
                    print(json.dumps({"failed": [scene, lib or "this build", res.returncode, res.stderr[-2000:]], "runs": runs}))
                    return 1
                one = json.loads(res.stdout.strip().splitlines()[-1])
                one["round"] = r
                runs.append(one)
    line = json.dumps({"frame": [W, H, SPP], "ring": RING, "bones": BONES, "influences": J, "runs": runs})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

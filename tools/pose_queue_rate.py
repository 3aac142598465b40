#!/usr/bin/env python3
"""What the queued pose commit (ft_scene_commit_moved_enqueue) is worth to a host that moves an object every frame.
Two scenes at 1920 x 1080 x 16: the full-size stand-in mesh (bunny_synth_full.ply, 69.6 K faces) as `bspMesh 0` under a transform node
and one directional light (tools/moved_commit_rate.py's scene and view), sliding; and hollow-sphere built by hand (its 25 CSG items of
primitives inside the shell, reflectance 0.4, one point light) with the sphere of its middle item sliding inside its cube.
`steps` steps of { translate, commit, ft_render_enqueue_into RGBA8 into a ring of page-locked frames }, the wall time of every step, then
one wait.  Three ways, each a context of its own:
  floor      no commit at all: the same frame queued every step
  blocking   ft_scene_commit_moved under "moved_in_place" 1: what the library could do before
  queued     ft_scene_commit_moved_enqueue
Per way the median step with min, max and the 10th / 90th percentile, the wall time per step over the whole run with the final wait, and
what ft_debug_pose_queue counted.
The driver (no --child) runs every (scene, library) pair as a process of its own under its own time limit, `rounds` rounds, this build
and - with --parent-lib - an older library in turn (it runs floor and blocking alone there), and stops at the first failure.  It prints
one JSON line and, with --out, writes it to a file.  Run on the GPU box."""
import argparse, json, math, os, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 16
RING = 8
SCENES = ("bunny", "hollow-sphere")
CHILD_LIMIT_S = 240


def stats(v):
    s = sorted(v)
    return {"median": round(statistics.median(s), 4), "min": round(s[0], 4), "max": round(s[-1], 4),
            "p10": round(s[len(s) // 10], 4), "p90": round(s[(9 * len(s)) // 10], 4)}


def child(scene, steps, warm):
    import functracer_amd as ft
    jit = ft.jitter_pattern(SPP)
    if scene == "bunny":
        with open(os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")) as f:
            tris = np.ascontiguousarray(ft.parse_ply(f.read()).reshape(-1, 9))
        p = tris.reshape(-1, 3) * 8.0
        centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
        cam = ft.make_camera(tuple(centre + np.array([0.0, 0.6, -2.2])), tuple(centre), (0, 1, 0), np.radians(50.0), 16.0 / 9.0)

        def pose(k):
            return [("scale", (8.0, 8.0, 8.0)), ("translate", (0.002 * (k % 50), 0.0, -0.001 * (k % 50)))]

        def build(ctx):
            ctx.clear()
            node = ctx.transform(pose(0), ctx.bsp_mesh(0, tris))
            ctx.set_objects(ctx.group([ctx.material(node, colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
            ctx.add_directional((-3.0, -2.0, 3.0), (1, 1, 1))
            ctx.commit()
            return node
    else:
        cam = ft.make_camera((5.7, 5.7, -5.7), (0, 0, 4), (0, 1, 0), math.radians(60.0), 1.0)
        colours = ((1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1))

        def pose(k):
            return [("scale", 0.65), ("translate", (0.004 * (k % 50) - 0.1, 0.0, 0.0))]

        def build(ctx):
            ctx.clear()
            items = [ctx.material(ctx.subtract(ctx.scale(11.0, ctx.primitive(ft.SPHERE)), ctx.scale(10.0, ctx.primitive(ft.SPHERE))), colour=(0.4, 0.4, 0.4))]
            node = None
            for row, y in enumerate((2.6, 1.3, 0.0, -1.3, -2.6)):
                for col, x in enumerate((-2.6, -1.3, 0.0, 1.3, 2.6)):
                    ball = ctx.transform(pose(0), ctx.primitive(ft.SPHERE))
                    if row == 2 and col == 2:
                        node = ball
                    op = ctx.subtract if (row + col) % 2 == 0 else ctx.intersect
                    items.append(ctx.material(ctx.translate((x, y, 0.0), op(ctx.primitive(ft.CUBE), ball)), colour=colours[col], reflectance=0.4, shineyness=10.0))
            ctx.set_objects(ctx.group(items))
            ctx.add_positional((0, 0, -8), (1, 0.01, 0.02), (1, 1, 1))
            ctx.commit()
            return node

    queued_known = hasattr(ft.hip_lib(), "ft_scene_commit_moved_enqueue")
    ways = ["floor", "blocking"] + (["queued"] if queued_known else [])
    ring = [ft.PinnedArray((H, W, 4), np.uint8) for _ in range(RING)]
    out = {"scene": scene, "steps": steps, "library": "FT_HIP_LIB" if os.environ.get("FT_HIP_LIB") else "this build", "ways": {}}
    small = {}
    for way in ways:
        ctx = ft.Context(0)
        ctx.set_option("moved_in_place", 1)
        node = build(ctx)
        commit = {"floor": None, "blocking": ctx.commit_moved, "queued": getattr(ctx, "commit_moved_enqueue", None)}[way]

        def step(k):
            if commit:
                ctx.set_transform(node, pose(k))
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
        if way == "queued":
            out["ways"][way]["pose_queue"] = ctx.pose_queue()
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
    line = json.dumps({"frame": [W, H, SPP], "ring": RING, "runs": runs})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

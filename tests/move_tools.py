"""Moved transforms committed in place (option "moved_in_place"): three shadow cases of tests/shadow_tools.py built the
way light_tools.build builds them, but with every caster and the receiver under a transform node whose handle is kept; the hand scene of
tests/test_temporal_motion.py; the pose sequences of each; and the oracle's view of every step.

A pose is a dict {node key: transform list} that names the whole list of every node that can move (a caster's part index, "receiver";
the hand scene's "sphere", "cube", "mesh", "operand"), so `build(b, case, pose)` makes from scratch the scene `move(ctx, handles, pose)`
moves a committed one to.  Step 0 is the case as shadow_tools.build poses it; a caster without a transform there stands under a
translation by zero."""
import functools
import math

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import light_tools as L
from . import shadow_tools as S
from . import walk_tools as W
from . import test_temporal_motion as M

NAMES = ("multi-leaf", "two_clusters", "blob(65)-mirror")
IDENTITY = [("translate", (0.0, 0.0, 0.0))]
AXIS = (2.0, 1.0, -1.5)                                             # not parallel to a light of any case (test_axis_is_parallel_to_no_light)
TURNS = (1.0, 30.0, 90.0, 180.0)                                    # degrees
SPP = 4
# the casters that move: of multi-leaf the 8-triangle blob and the 65-triangle one that stands under rotate + scale + translate
MOVERS = {"multi-leaf": (0, 3), "two_clusters": (0,), "blob(65)-mirror": (0,)}
TRANSLATE, TURN, SCALE, TO_IDENTITY, SINGULAR, ORIGINAL = "translate", "turn", "scale", "identity", "singular", "original"


def base_pose(case):
    recv_ops, _ = S.geometry(case)
    pose = {k: list(ops) if ops else list(IDENTITY) for k, (_, ops, _) in enumerate(case.parts)}
    pose["receiver"] = list(recv_ops)
    return pose


def centre_of(case, part):
    """The world position of the middle of a caster's dense part, in the case's own pose."""
    m, t = W.matrix(case.parts[part][1])
    c, r = S.mesh_ball(case.parts[part][0])
    return m @ c + t, r * float(np.linalg.svd(m, compute_uv=False).max())


def about(c, inner):
    """`inner` applied about the point c."""
    return [("translate", tuple(float(-x) for x in c))] + list(inner) + [("translate", tuple(float(x) for x in c))]


@functools.lru_cache(maxsize=None)
def sequence(name):
    """[(kind, what, pose)] of a case, step 0 first."""
    case = S.CASES[name]
    base = base_pose(case)
    movers = MOVERS[name]
    _, view = S.geometry(case)

    def posed(change, only=None):
        pose = {k: list(v) for k, v in base.items()}
        for part in movers if only is None else only:
            c, r = centre_of(case, part)
            pose[part] = change(part, c, r)
        return pose

    slide = lambda f: (lambda part, c, r: base[part] + [("translate", (f * r, 0.0, -0.6 * f * r))])
    steps = [(ORIGINAL, "original", posed(lambda part, c, r: base[part]))]
    moved = posed(slide(0.35))
    n = -np.asarray(W.matrix(base["receiver"])[0] @ np.array([0.0, 1.0, 0.0]))   # away from the lights
    moved["receiver"] = base["receiver"] + [("translate", tuple(float(x) for x in 0.05 * centre_of(case, movers[0])[1] * n))]
    steps.append((TRANSLATE, "casters and receiver slid", moved))
    for deg in TURNS:
        steps.append((TURN, f"turned {deg:g} degrees", posed(lambda part, c, r: base[part] + about(c, [("rotate", AXIS, math.radians(deg))]))))
    steps.append((SCALE, "scaled unevenly", posed(lambda part, c, r: base[part] + about(c, [("scale", (1.25, 0.8, 1.1))]))))
    steps.append((TO_IDENTITY, "a list becomes the identity", posed(lambda part, c, r: list(IDENTITY), only=movers[-1:])))
    steps.append((TRANSLATE, "and leaves it again", posed(slide(-0.3))))
    steps.append((SINGULAR, "singular", posed(lambda part, c, r: base[part] + about(c, [("scale", (1.0, 0.0, 1.0))]), only=movers[:1])))
    steps.append((SCALE, "regular again", posed(lambda part, c, r: base[part] + about(c, [("scale", (1.0, 0.5, 1.0))]), only=movers[:1])))
    steps.append((ORIGINAL, "original again", posed(lambda part, c, r: base[part])))
    return steps


def build(b, case, pose, lights=None, tris=None):
    """light_tools.build with every caster and the receiver under a transform node of `pose`.  Returns the handles: {key: transform node}
    and, under "meshes", the bspMesh node of every part.  tris: {part: vertices} instead of the catalogue's."""
    lights = L.initial(case) if lights is None else lights
    b.clear()
    handles, items, node, meshes = {}, [], None, []
    for k, (mesh, ops, kind) in enumerate(case.parts):
        if kind != "same":
            node = b.bsp_mesh(0, (tris or {}).get(k, S.mesh_tris(mesh)).reshape(-1, 9))
        meshes.append(node)
        handles[k] = b.transform(list(pose[k]), node)
        item = b.material(handles[k], colour=S.MESH_COLOUR)
        items.append(b.ignore_light(item) if kind == "unlit" else item)
    handles["receiver"] = b.transform(list(pose["receiver"]), b.primitive(ft.SQUARE))
    items.append(b.material(handles["receiver"], colour=S.RECEIVER_COLOUR))
    b.set_objects(b.group(items))
    L.add_lights(b, lights)
    b.commit()
    handles["meshes"] = meshes
    return handles


def move(ctx, handles, pose, commit=True):
    """set_transform for every node of the pose, then commit_moved."""
    for key, ops in pose.items():
        ctx.set_transform(handles[key], list(ops))
    if commit:
        ctx.commit_moved()


# ---------------------------------------------------------------------------------------------------------------- the hand scene
HAND = "hand"


@functools.lru_cache(maxsize=None)
def hand_sequence():
    """[(kind, what, pose)] of test_temporal_motion.py's hand scene (its _build / _pose), step 0 = _pose(0)."""
    base = M._pose(0.0)
    mesh_at = (-4.9, 3.2, 0.5)

    def posed(**lists):
        pose = {k: list(v) for k, v in base.items()}
        pose.update({k: list(v) for k, v in lists.items()})
        return pose

    steps = [(ORIGINAL, "original", posed())]
    steps.append((TRANSLATE, "sphere and mesh slid", posed(sphere=[("translate", (-3.4, 1.0, -2.0))], mesh=base["mesh"][:2] + [("translate", (-4.6, 3.1, 0.4))])))
    for deg in TURNS:
        steps.append((TURN, f"turned {deg:g} degrees", posed(mesh=base["mesh"][:2] + [("rotate", AXIS, math.radians(deg)), ("translate", mesh_at)],
                                                           cube=[("rotate", (0, 1, 0), math.radians(20.0 + deg))] + base["cube"][1:])))
    steps.append((SCALE, "scaled unevenly", posed(mesh=[("scale", (8.0, 6.0, 9.0))] + base["mesh"][1:], cube=[base["cube"][0], ("scale", (2.0, 1.1, 0.7)), base["cube"][2]],
                                                 operand=[("scale", (0.8, 0.6, 0.8))] + base["operand"][1:])))
    steps.append((TO_IDENTITY, "a list becomes the identity", posed(sphere=list(IDENTITY))))
    steps.append((TRANSLATE, "and leaves it again", posed(sphere=[("translate", (-4.3, 1.2, -1.5))])))
    steps.append((SINGULAR, "singular", posed(mesh=[("scale", (1.0, 0.0, 1.0))] + base["mesh"])))
    steps.append((SCALE, "regular again", posed(mesh=[("scale", (1.0, 0.5, 1.0))] + base["mesh"])))
    steps.append((ORIGINAL, "original again", posed()))
    return steps


def steps_of(name):
    return hand_sequence() if name == HAND else sequence(name)


def build_any(b, name, pose, **kw):
    """The scene of `name` (a case or HAND) at `pose`; returns the handles."""
    if name == HAND:
        return M._build(b, pose)
    return build(b, S.CASES[name], pose, **kw)


def render(c, name, spp=SPP, **kw):
    if name == HAND:
        return c.render(M._camera(), M.W, M.Hh, spp, S.jitter(spp), **kw)
    view = S.view_of(S.CASES[name])
    return c.render(W.camera(view), view.w, view.h, spp, S.jitter(spp), tiles=view.tiles, **kw)


def render_aov(c, name):
    if name == HAND:
        return c.render_aov(M._camera(), M.W, M.Hh, 1, S.jitter(1))
    view = S.view_of(S.CASES[name])
    return c.render_aov(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)


# ---------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def oracle_steps(name):
    """Per step of a case: (receiver pixels in view that some directional light leaves in shadow, the oracle's 1-sample frame)."""
    case = S.CASES[name]
    view = S.view_of(case)
    lights = L.initial(case)
    out = []
    for _, _, pose in sequence(name):
        orc = O.Oracle()
        build(orc, case, pose)
        o, d, _, _ = W.pixel_rays(view)
        hit, _, p, n, col = orc.closest(o + S.SLIGHT_OFFSET * d, d)
        hit = hit.astype(bool)
        receiver = hit & (np.abs(col - np.array(S.RECEIVER_COLOUR)).max(axis=1) < 1e-9)
        origin = p + S.SLIGHT_OFFSET * n
        dark = np.zeros(len(hit), dtype=bool)
        for l in lights:
            if l[0] != "dir":
                continue
            v = np.asarray(l[1], dtype=np.float64)
            dark[receiver] |= orc.blocked(origin[receiver], np.broadcast_to(-v, origin[receiver].shape).copy(), np.full(int(receiver.sum()), 1e300)).astype(bool)
        frame, _ = orc.render(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
        orc.close()
        out.append((int(dark.sum()), frame))
    return out


@functools.lru_cache(maxsize=None)
def oracle_hand_frames():
    """The oracle's 1-sample frame of every step of the hand scene."""
    out = []
    for _, _, pose in hand_sequence():
        orc = O.Oracle()
        M._build(orc, pose)
        frame, _ = orc.render(M._camera(), M.W, M.Hh, 1, S.jitter(1))
        orc.close()
        out.append(frame)
    return out


# ---------------------------------------------------------------------------------------------------------------- the three-cube union
def union_pose(b_deg=30.0, c_deg=0.0, whole=(0.0, 1.0, 0.0), whole_deg=0.0):
    """Three cubes in one union, each under its own transform, the union under one more.  A and C stand along the axes, B is turned about y:
    at most five face directions.  C turned about x as well takes the item past the six a cull record holds."""
    return {"a": [("translate", (-0.4, 0.0, 0.0))], "b": [("rotate", (0, 1, 0), math.radians(b_deg)), ("translate", (0.4, 0.1, 0.0))],
            "c": ([("rotate", (1, 0, 0), math.radians(c_deg))] if c_deg else []) + [("translate", (0.0, 0.5, 0.3))],
            "whole": ([("rotate", (0, 1, 0), math.radians(whole_deg))] if whole_deg else []) + [("translate", tuple(whole))]}


UNION_CAM = dict(o=(1.5, 3.0, -5.0), look_at=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov=40.0, w=96, h=72)


def build_union(b, pose, extra_cubes=()):
    """The union over a square under one directional light; extra_cubes: transform lists of further top-level cubes (their face directions
    count towards the scene-wide table of 32).  Returns the handles, the extra cubes' under ("extra", k)."""
    b.clear()
    hd = {k: b.transform(list(pose[k]), b.primitive(ft.CUBE)) for k in ("a", "b", "c")}
    hd["whole"] = b.transform(list(pose["whole"]), b.union(b.union(hd["a"], hd["b"]), hd["c"]))
    items = [b.material(hd["whole"], colour=(0.7, 0.5, 0.4)),
             b.material(b.transform([("scale", (8.0, 1.0, 8.0)), ("translate", (-4.0, 0.0, -4.0))], b.primitive(ft.SQUARE)), colour=(0.6, 0.6, 0.6))]
    for k, ops in enumerate(extra_cubes):
        hd[("extra", k)] = b.transform(list(ops), b.primitive(ft.CUBE))
        items.append(b.material(hd[("extra", k)], colour=(0.3, 0.5, 0.8)))
    b.set_objects(b.group(items))
    b.add_directional((0.3, -1.0, 0.2), (1.0, 1.0, 1.0))
    b.commit()
    return hd


def union_camera():
    return ft.make_camera(UNION_CAM["o"], UNION_CAM["look_at"], UNION_CAM["up"], math.radians(UNION_CAM["fov"]), UNION_CAM["w"] / UNION_CAM["h"])

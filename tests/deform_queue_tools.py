"""Queued deform commits (ft_scene_commit_deformed_enqueue): the scene, the poses and the edits of
tests/test_deform_queue.py, and the oracle's view of each pose.

The scene is a tube of 312 triangles ("arm") skinned to four bones over a receiver plane of 72 triangles, both `bspMesh 0` meshes, under
one directional and one point light.  The arm stands under a transform node, so that a pose commit can slide it.  A pose k bends the arm:
bone b turns by b * ANGLE * k about the z axis through a pivot on the arm's axis.  The plane ripples with a phase of its own.

An edit KIND says how pose k reaches the library: a matrix palette ("bones"), a dual-quaternion palette ("dq"), weights of two key
shapes ("weights"), weights under a palette ("weights+bones"), explicit vertices ("verts") and a matrix palette under "skin_on_device" 0
("host-skin").  expected(kind, k) is what a fresh context is handed instead: the vertices from functracer_amd.skin_blend, skin_blend_dq
and morph_blend."""
import functools
import math

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

STEPS = 12                      # more than the geometry sets a device may hold (9)
FRAME_SLOTS = 4                 # ft_context::kSlots: a device's frames in flight
KINDS = ("bones", "weights", "dq", "weights+bones", "verts", "host-skin")
SEGMENTS, RINGS, BONES, J = 12, 14, 4, 2
LENGTH, RADIUS = 3.0, 0.35
ANGLE = 0.045                   # radians per bone index and pose
FRAMES = {4: (96, 72), 16: (160, 90)}                               # spp -> (width, height)
MIN_CHANGED_FRACTION = 0.01


def _quads(p00, p01, p10, p11):
    return [np.concatenate([p00, p10, p11]), np.concatenate([p00, p11, p01])]


@functools.lru_cache(maxsize=None)
def arm():
    """(tris [312, 9], index [312, 3, 2], weight [312, 3, 2]): a tube about the y axis from y = 0 to LENGTH; a corner at height y is shared
    by the two bones around it in proportion, so that a bend is smooth."""
    def point(r, s):
        a = 2.0 * math.pi * s / SEGMENTS
        return np.array([RADIUS * math.cos(a), LENGTH * r / (RINGS - 1), RADIUS * math.sin(a)])
    tris = []
    for r in range(RINGS - 1):
        for s in range(SEGMENTS):
            tris += _quads(point(r, s), point(r, s + 1), point(r + 1, s), point(r + 1, s + 1))
    tris = np.ascontiguousarray(np.array(tris))
    y = tris.reshape(-1, 3)[:, 1]
    f = np.clip(y / LENGTH * (BONES - 1), 0.0, BONES - 1 - 1e-9)
    lo = np.floor(f).astype(np.int32)
    index = np.stack([lo, lo + 1], axis=1).reshape(-1, 3, J)
    weight = np.stack([1.0 - (f - lo), f - lo], axis=1).reshape(-1, 3, J)
    return tris, np.ascontiguousarray(index), np.ascontiguousarray(weight)


@functools.lru_cache(maxsize=None)
def plane(k=0):
    """The receiver [72, 9] at ripple phase k: a 6 x 6 grid of quads over x, z in [-4, 4] about y = -0.5."""
    n, half = 6, 4.0

    def point(i, j):
        x, z = -half + 2.0 * half * i / n, -half + 2.0 * half * j / n
        return np.array([x, -0.5 + 0.25 * math.sin(0.9 * x + 0.7 * k) * math.cos(0.6 * z - 0.4 * k) * (1.0 if k else 0.0), z])
    tris = []
    for i in range(n):
        for j in range(n):
            tris += _quads(point(i, j), point(i + 1, j), point(i, j + 1), point(i + 1, j + 1))   # (wound so that the normals point up)
    return np.ascontiguousarray(np.array(tris))


def _turns(k):
    """Per bone (angle about z, pivot)."""
    return [(b * ANGLE * k, np.array([0.0, LENGTH * max(b - 1, 0) / (BONES - 1), 0.0])) for b in range(BONES)]


def palette(k):
    """[BONES, 12]: x -> R (x - p) + p."""
    out = np.zeros((BONES, 3, 4))
    for b, (a, p) in enumerate(_turns(k)):
        R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        out[b, :, :3] = R
        out[b, :, 3] = p - R @ p
    return out.reshape(BONES, 12)


def palette_dq(k):
    """[BONES, 8]: the same turns as dual quaternions."""
    rot, tr = [], []
    for a, p in _turns(k):
        R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        rot.append([math.cos(a / 2.0), 0.0, 0.0, math.sin(a / 2.0)])
        tr.append(p - R @ p)
    return ft.dual_quaternions(np.array(rot), np.array(tr))


@functools.lru_cache(maxsize=None)
def targets():
    """[2, 312, 9]: the arm bent as pose 8 bends it, and the arm swollen about its axis."""
    base, index, weight = arm()
    swollen = base.reshape(-1, 3) * np.array([1.6, 1.0, 1.6])
    return np.ascontiguousarray(np.stack([ft.skin_blend(base, index, weight, palette(8)), swollen.reshape(-1, 9)]))


def weights(k):
    return np.array([0.11 * k, 0.04 * k])


def expected(kind, k):
    """The arm's vertices [312, 9] at pose k as edit kind `kind` declares them."""
    base, index, weight = arm()
    if kind in ("bones", "verts", "host-skin"):
        return ft.skin_blend(base, index, weight, palette(k))
    if kind == "dq":
        return ft.skin_blend_dq(base, index, weight, palette_dq(k))
    if kind == "weights":
        return ft.morph_blend(base, targets(), weights(k))
    assert kind == "weights+bones"
    return ft.skin_blend(ft.morph_blend(base, targets(), weights(k)), index, weight, palette(k))


def slide(k):
    """The arm's transform at pose step k (a translation: queued whatever "light_space_shadows" says)."""
    return [("translate", (0.12 * k, 0.0, -0.05 * k))]


LIGHTS = (("dir", (1.0, -2.0, 1.0), (1.0, 1.0, 1.0)), ("point", (2.0, 3.0, -2.0), (1.0, 0.1, 0.01), (0.5, 0.5, 1.0)))


def point_light(k):
    return (2.0 - 0.3 * k, 3.0, -2.0 + 0.2 * k), (1.0, 0.1, 0.01), (0.5 + 0.03 * k, 0.5, 1.0 - 0.03 * k)


def build(b, arm_tris, plane_tris, ops=None, point=None):
    """The scene in builder `b` (a Context or the oracle), committed.  Returns the handles."""
    b.clear()
    hd = {"arm": b.bsp_mesh(0, np.asarray(arm_tris).reshape(-1, 9)), "plane": b.bsp_mesh(0, np.asarray(plane_tris).reshape(-1, 9))}
    hd["xf"] = b.transform(ops if ops is not None else slide(0), b.material(hd["arm"], colour=(0.9, 0.5, 0.2), shineyness=4.0))
    b.set_objects(b.group([hd["xf"], b.material(hd["plane"], colour=(0.5, 0.7, 0.9))]))
    b.add_directional(LIGHTS[0][1], LIGHTS[0][2])
    b.add_positional(*(point if point is not None else LIGHTS[1][1:]))
    b.commit()
    return hd


def prepare(ctx, kind):
    """The work context of edit kind `kind`: the scene at rest, the skin and the key shapes the kind needs, and the one blocking
    commit_deformed that makes the refit's tables (pose 0).  Returns the handles."""
    base, index, weight = arm()
    ctx.set_option("skin_on_device", 0 if kind == "host-skin" else 1)
    hd = build(ctx, base, plane())
    if kind in ("weights", "weights+bones"):
        ctx.set_mesh_targets(hd["arm"], targets())
    if kind in ("bones", "dq", "weights+bones", "host-skin"):
        ctx.set_mesh_skin(hd["arm"], index, weight)
    edit(ctx, hd, kind, 0)
    ctx.commit_deformed()
    return hd


def edit(ctx, hd, kind, k):
    """Pose k of the arm handed to the library the way `kind` says; nothing is committed."""
    if kind in ("weights", "weights+bones"):
        ctx.set_mesh_weights(hd["arm"], weights(k))
    if kind in ("bones", "weights+bones", "host-skin"):
        ctx.set_mesh_bones(hd["arm"], palette(k))
    if kind == "dq":
        ctx.set_mesh_bones_dq(hd["arm"], palette_dq(k))
    if kind == "verts":
        ctx.set_mesh_triangles(hd["arm"], expected(kind, k))


def camera(spp):
    w, h = FRAMES[spp]
    return ft.make_camera((3.4, 3.0, -6.2), (0.2, 1.0, 0.0), (0, 1, 0), math.radians(50.0), w / h)


def frame_args(spp):
    w, h = FRAMES[spp]
    return camera(spp), w, h, spp, ft.jitter_pattern(spp)


def changed(a, b):
    """Pixels in which two frames differ."""
    return int((np.any(a != b, axis=2) & ~(np.isnan(a).all(axis=2) & np.isnan(b).all(axis=2))).sum())


@functools.lru_cache(maxsize=None)
def oracle_frames(kind, plane_too=False):
    """The oracle's 1-sample 96 x 72 frame of poses 0 .. STEPS of edit kind `kind`; plane_too: the two-mesh sequence of the carry test,
    where even steps pose the arm and odd steps ripple the plane."""
    cam, w, h, _, _ = frame_args(4)
    out = []
    for k in range(STEPS + 1):
        orc = O.Oracle()
        ka, kp = (two_mesh_state(k) if plane_too else (k, 0))
        build(orc, expected(kind, ka), plane(kp))
        out.append(orc.render(cam, w, h, 1, ft.jitter_pattern(1))[0])
        orc.close()
    return out


def two_mesh_state(k):
    """(arm pose, plane phase) after step k of the carry sequence: step k edits the arm when k is even, the plane when it is odd."""
    return 2 * (k // 2), (2 * ((k + 1) // 2) - 1 if k > 0 else 0)


def pending_at_last_call(frames_queued_before):
    """Frames the host still has pending when the commit of the last step returns, from the frame driver's rule alone: with one frame
    queued per step every frame queued so far is pending until the FRAME_SLOTS slots are full, and FRAME_SLOTS of them from then on.  A
    queued commit retires none."""
    return min(frames_queued_before, FRAME_SLOTS)

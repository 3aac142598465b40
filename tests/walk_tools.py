"""Scenes, views and readers for tests/test_coherent_walks.py: meshes and cameras at which the mesh walks of a coherent wave
(ft_kernels.hip: mesh_bsp_packet, mesh_bsp_narrow, mesh_bvh_packet and their any-hit halves) can go wrong, each a function of a builder
so that the oracle, a host-only context and the device build the same one.

Tall trees.  `tall(n, sign)` is n triangles whose boxes are sign * 3^k * (1 +- 0.1) on every axis, k = 0 .. n - 1.  BspMesh.compile cuts
the longest axis of the bounds at its middle: the largest triangle lies alone on one side, everything else on the other, and nothing is
clipped.  So the tree has exactly n - 1 branch levels, one leaf of one triangle per level.  sign = +1: the largest triangle is above the
plane, which is the LEFT child, and the rest goes RIGHT: a right-deep tree, in which a walk that descends right and keeps the left
children pending holds one entry per level.  sign = -1 is the mirror image: left-deep, one pending entry at any time.  The layout
is the same at every scale, so a camera near triangle j sees what a camera near triangle 0 sees, 3^j times larger."""
import functools
import math
from collections import namedtuple

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import bvh_tools as B

INT32_MIN = -2 ** 31
WAVE_STACK = 64                                   # entries of a WaveStack: one per lane
PACKET_LEVELS = 40                                # the tallest BSP that gets two-level records (build_bsp)
LDS_STACK_ENTRIES = 160                           # 160 KiB of LDS / (256 lanes * 4 bytes): the tallest per-lane stack a commit accepts
SLIGHT_OFFSET = 1e-4                              # Shading.fs:129

# name, camera (origin, look_at, fov in degrees), frame width and height, tile list or None, transform of the mesh or None
View = namedtuple("View", "name o look fov w h tiles ops")


def tall(n, sign):
    return np.stack([B._boxed(np.full(3, sign * 3.0 ** k), 0.1 * 3.0 ** k) for k in range(n)])


def tall_triangle_of(p):
    """Which triangle of a tall mesh the point p lies on: triangle k lives inside 3^k * [0.9, 1.1] on every axis."""
    return np.rint(np.log(np.abs(p).max(axis=-1)) / math.log(3.0)).astype(np.int64)


def camera(view):
    return ft.make_camera(tuple(view.o), tuple(view.look), (0, 1, 0), math.radians(view.fov), view.w / view.h)


def matrix(ops):
    """The 3x3 part and the offset of a transform list (first listed applied first), in numpy."""
    m, t = np.eye(3), np.zeros(3)
    for op in ops or []:
        if op[0] == "translate":
            t = t + np.asarray(op[1], dtype=np.float64)
            continue
        if op[0] == "scale":
            a = np.diag(np.broadcast_to(np.asarray(op[1], dtype=np.float64), (3,)))
        else:
            u = np.asarray(op[1], dtype=np.float64) / np.linalg.norm(op[1])
            k = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
            a = np.eye(3) + math.sin(op[2]) * k + (1 - math.cos(op[2])) * (k @ k)
        m, t = a @ m, a @ t
    return m, t


def build(b, tris, depth, ops=None, light=None):
    """One `bspMesh depth` of `tris` (under `ops`), a directional light and, with `light`, a point light of constant intensity there."""
    b.clear()
    node = b.bsp_mesh(depth, np.asarray(tris).reshape(-1, 9))
    if ops:
        node = b.transform(list(ops), node)
    b.set_objects(b.group([b.material(node, colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    b.add_directional((-1.0, -1.3, -0.8), (1, 1, 1))
    if light is not None:
        b.add_positional(tuple(light), (1.0, 0.0, 0.0), (0.5, 0.5, 1.0))
    b.commit()


def pixels_of(view):
    if view.tiles is None:
        return [(x, y) for y in range(view.h) for x in range(view.w)]
    return sorted({(x, y) for (x0, y0, tw, th) in view.tiles for y in range(max(0, y0), min(view.h, y0 + th)) for x in range(max(0, x0), min(view.w, x0 + tw))},
                  key=lambda p: (p[1], p[0]))


def pixel_rays(view):
    """The geometry rays of the view's tile pixels at jitter offset (0, 0): origins before slightOffset, directions, xs, ys."""
    cam, px = camera(view), pixels_of(view)
    o, d = np.zeros((len(px), 3)), np.zeros((len(px), 3))
    for k, (x, y) in enumerate(px):
        o[k], d[k] = O.ray_through_pixel(cam, view.w, view.h, x, y, 0.0, 0.0)
    return o, d, np.array([p[0] for p in px]), np.array([p[1] for p in px])


# ---------------------------------------------------------------------------------------------------------------- shallow shapes
SHALLOW = ("blob(7)", "blob(9)", "blob(65)", "flat", "flat_x", "degenerate", "identical", "concentric", "spanning", "two_clusters", "geometric")
SHALLOW_DEPTHS = (1, 2, 3, 5)
XF = [("rotate", (1.0, 2.0, 0.5), 0.7), ("scale", (1.3, 0.6, 0.9)), ("translate", (0.2, -0.1, 0.3))]
TILES = [(0, 0, 13, 9), (17, 5, 22, 19), (37, 30, 30, 30)]       # the last one hangs over the frame's edge

# bvh_tools.camera(centre, radius) - direction (0.9, 1.3, -3.6) from the target, 50 degrees - shows these meshes on 0.2 % .. 4 % of the
# frame: their triangles are small against their spread.  So the camera moved, on the oracle alone, until every view shows the mesh on 15 %
# .. 75 % of its pixels: it keeps that direction, and stands `dist` radii (1: bvh_tools.camera's own 3.93 radii) from a target - the centre
# ("c") or the centroid of a triangle - under a narrower field of view.  For the sparse blobs that is a close look at one or two triangles.
_DIR = np.array([0.9, 1.3, -3.6])
_OUTSIDE = {                                                        # name -> (target, dist, fov)
    "blob(7)": (0, 0.7 / 3.93, 5.0), "blob(9)": (1, 1.2 / 3.93, 5.0), "blob(65)": (10, 0.3 / 3.93, 30.0), "flat": ("c", 1.0, 18.0), "flat_x": ("c", 1.0, 5.0),
    "degenerate": (89, 2.0 / 3.93, 18.0), "identical": (280, 1.0, 10.0), "concentric": ("c", 1.0, 10.0), "spanning": (314, 0.7 / 3.93, 50.0),
    "two_clusters": (49, 1.0, 10.0), "geometric": (0, 1.2 / 3.93, 5.0),
}
# The eye of the inside view, strictly inside the mesh's bounds (asserted): the centre plus this fraction of the extent, a target, a field
# of view.  `flat` and `flat_x` have none: their box has no thickness, and from a point of their plane every triangle is seen edge-on.
_INSIDE = {                                                         # name -> (fraction of the extent, target, fov)
    "blob(7)": ((0.1, 0.1, -0.1), 5, 10.0), "blob(9)": ((0.02, -0.03, -0.3), 6, 10.0), "blob(65)": ((0.02, -0.03, -0.3), 10, 70.0),
    "degenerate": ((0.3, 0.3, 0.3), 21, 50.0), "identical": ((0.02, -0.03, -0.3), 280, 70.0), "concentric": ((0.1, 0.1, -0.1), 0, 50.0),
    "spanning": ((0.3, 0.3, 0.3), "c", 70.0), "geometric": ((0.1, 0.1, -0.1), 0, 18.0),
}


def _target(e, spec):
    """The centre of the bounds lies on the root's cut plane, and the rays of the frame's centre column would run along the cut between two
    clipped pieces, where a hit is decided by the last bit of a determinant (at bspMesh 0 the oracle hits there, at bspMesh 1 it slips
    through the crack): "c" is a point beside the centre."""
    return e.centre + e.radius * np.array([0.013, 0.021, 0.017]) if spec == "c" else e.tris[spec].mean(axis=0)


def shallow_views(name):
    """outside (a full frame whose width is no multiple of 8), inside (tiles), and the outside view again with the mesh under rotate +
    non-uniform scale and the camera's eye and target carried along."""
    e = B.catalogue()[name]
    spec, dist, fov = _OUTSIDE[name]
    target = _target(e, spec)
    eye = target + dist * e.radius * _DIR
    out = [View("outside", eye, target, fov, 76, 60, None, None)]
    if name == "two_clusters":                                      # beside the cluster at the origin, inside the bounds (0 .. 577)
        out.append(View("inside", np.array([0.02, 0.015, 0.01]), np.zeros(3), 30.0, 60, 52, TILES, None))
    elif name in _INSIDE:
        lo, hi = e.tris.reshape(-1, 3).min(axis=0), e.tris.reshape(-1, 3).max(axis=0)
        frac, spec, fov_in = _INSIDE[name]
        out.append(View("inside", e.centre + (hi - lo) * np.array(frac), _target(e, spec), fov_in, 60, 52, TILES, None))
    m, t = matrix(XF)
    out.append(View("transformed", m @ eye + t, m @ target + t, fov, 52, 44, None, XF))
    return out


def shallow_light(name):
    """The point light of the plane views (which trace no shadow ray)."""
    e = B.catalogue()[name]
    return e.centre + e.radius * np.array([0.05, 0.12, -0.08])


# The shadow frames have views and point lights of their own, found on the oracle alone: an eye, a target, a field of view and a light such
# that some primary hits have an occluder between them and the light and others have one only beyond the light (shadow_counts: 0 < near <
# far), which is what an any-hit walk that skips a leaf, or forgets its max_dist bound, gets wrong.
#   NO_SELF_SHADOW: `flat` and `flat_x` are coplanar and `identical` is 300 times one triangle: no triangle of theirs stands between
#   another and any light.  Their frames only show that the any-hit walks report no occluder where there is none.
#   BEFORE_ONLY: the 7 and 9 sparse triangles of the two small blobs.  A search over every ordered pair of triangles as (seen, occluder),
#   three light distances behind the occluder and four eyes each found hits shadowed before the light, and none that also had hits
#   shadowed only beyond it: these frames guard a skipped leaf, not the max_dist bound.
NO_SELF_SHADOW = ("flat", "flat_x", "identical")
BEFORE_ONLY = ("blob(7)", "blob(9)")
_SHADOW = {                                                         # name -> (eye, target, fov, light)
    "blob(65)": ((-0.0059, 2.0036, 2.959), (0.4696, 0.6208, 0.312), 8.0, (0.4713, 0.7757, -0.2641)),
    "degenerate": ((-0.105, -7.6149, 1.22), (-0.0575, 1.1598, 0.2155), 8.0, (-0.5649, -1.0564, -0.0718)),
    "concentric": ((-5.5399, -0.6177, 3.0794), (-0.2188, -0.2188, -0.2188), 16.0, (-0.455, -0.6692, -0.6819)),
    "spanning": ((5.3461, -2.0814, -3.5997), (-0.88, -1.4659, -0.6238), 8.0, (-0.6059, 0.6093, 0.412)),
    # the far cluster, lit from a point on the diagonal between the clusters: the cluster at the origin lies beyond the light
    "two_clusters": ((577.3484, 577.3107, 577.347), (577.3518, 577.3504, 577.3505), 8.0, (173.207, 173.2025, 173.2067)),
    # beside the triangle at 1/256 looking out along the diagonal: the triangle at 1/16 and, around it, the one at 1; the light between 1/256 and 1/16
    "geometric": ((0.0091, -0.0071, 0.002), (0.5, 0.5, 0.5), 20.0, (0.012, 0.01248, 0.01176)),
    "blob(7)": ((0.4631, -0.001, 0.1771), (0.441, -0.1161, 0.5898), 15.0, (0.3238, 1.1939, -0.5126)),
    "blob(9)": ((0.6268, -0.3459, 0.412), (0.4694, -0.0941, 0.6485), 15.0, (0.6605, -0.0438, -1.7162)),
}


def shadow_view(name):
    if name in NO_SELF_SHADOW:
        return shallow_views(name)[0]._replace(name="shadow", w=60, h=52), shallow_light(name)
    eye, look, fov, light = _SHADOW[name]
    return View("shadow", np.array(eye), np.array(look), fov, 60, 52, None, None), np.array(light)


# ---------------------------------------------------------------------------------------------------------------- tall trees
TALL_SIZES = (41, 42, 64, 65, 66, 67)


def tall_views(n, sign):
    """small: an eye beside triangle 0 looking out along the diagonal: triangles 1, 2, 3, ... nest around the frame's centre, the small
    near ones in front.  large: the same eye beside triangle n - 4, 3^(n - 4) times further out: the three largest triangles."""
    eye, look, s = np.array([0.45, -0.35, 0.1]), np.full(3, 9.0), 3.0 ** (n - 4)
    return [View("small", sign * eye, sign * look, 16.0, 68, 60, None, None),
            View("large", sign * s * eye, sign * s * look, 16.0, 52, 44, [(0, 0, 52, 18), (5, 18, 43, 30)], None)]


def tall_light(view_name, n, sign):
    """Between the second and the third triangle the view shows: seen from the triangles further out, the nearer ones lie beyond it."""
    s = 1.0 if view_name == "small" else 3.0 ** (n - 4)
    return sign * s * np.array([5.5, 5.7, 5.4])


# ---------------------------------------------------------------------------------------------------------------- axis-parallel lanes
# The eye looks along +z from a point whose offset to the target is exact, so the camera's frame is the model's axes; with pixel_width =
# width / (res_v - 1) and pixel_height = height / (res_h - 1) (sic, Image.fs:71-72) the pixel column res_v / 2 - 1 has x = 0 and the pixel
# row res_h / 2 - 1 has y = 0 when both are even - exactly or not is for test_axis_views_hold_exactly_axis_parallel_rays to say.
AXIS_CASES = [("blob(257)", 0), ("flat", 0), ("blob(65)", 3)]
AXIS_EYE = {"blob(257)": 4.0, "flat": 4.0, "blob(65)": 2.5}        # how far in front of the target the eye stands


def axis_view(name):
    e = B.catalogue()[name]
    c = np.round(e.centre * 8.0) / 8.0
    return View("axis", c - np.array([0.0, 0.0, AXIS_EYE[name]]), c, 40.0, 60, 60, None, None)


# ---------------------------------------------------------------------------------------------------------------- the oracle's answers
@functools.lru_cache(maxsize=None)
def reference(kind, name, depth, view_name):
    """closest() of the oracle on the view's rays (after slightOffset), computed once and shared: (view, light, tris, rays, answer)."""
    view, light, tris = case(kind, name, view_name)
    orc = O.Oracle()
    build(orc, tris, depth, view.ops, light)
    o, d, xs, ys = pixel_rays(view)
    ans = orc.closest(o + SLIGHT_OFFSET * d, d)
    orc.close()
    for a in (o, d, xs, ys) + tuple(ans):
        a.setflags(write=False)
    return {"view": view, "light": light, "tris": tris, "o": o, "d": d, "xs": xs, "ys": ys, "closest": ans}


@functools.lru_cache(maxsize=None)
def reference_frame(kind, name, depth, view_name, w, h):
    view, light, tris = case(kind, name, view_name)
    view = view._replace(w=w, h=h, tiles=None)
    orc = O.Oracle()
    build(orc, tris, depth, view.ops, light)
    frame, _ = orc.render(camera(view), w, h, 2, ft.jitter_pattern(2))
    orc.close()
    frame.setflags(write=False)
    return view, light, tris, frame


def shadow_counts(ref, depth):
    """On the oracle: (primary hits, those whose ray to the point light is blocked before the light, those blocked anywhere along it)."""
    orc = O.Oracle()
    build(orc, ref["tris"], depth, ref["view"].ops, ref["light"])
    m = ref["closest"][0].astype(bool)
    p = ref["closest"][2][m]
    d = ref["light"] - p
    dist = np.linalg.norm(d, axis=1)
    d = d / dist[:, None]
    near, far = orc.blocked(p + SLIGHT_OFFSET * d, d, dist), orc.blocked(p + SLIGHT_OFFSET * d, d, np.full(len(p), 1e300))
    orc.close()
    return int(m.sum()), int(near.sum()), int(far.sum())


def case(kind, name, view_name):
    """(view, point light, triangles) of a case.  kind 'shallow': name a catalogue entry; 'tall': name (n, sign); 'axis': a catalogue entry."""
    if kind == "tall":
        n, sign = name
        view = {v.name: v for v in tall_views(n, sign)}[view_name]
        return view, tall_light(view_name, n, sign), tall(n, sign)
    e = B.catalogue()[name]
    if kind == "shallow" and view_name == "shadow":
        view, light = shadow_view(name)
        return view, light, e.tris
    view = axis_view(name) if kind == "axis" else {v.name: v for v in shallow_views(name)}[view_name]
    m, t = matrix(view.ops)
    return view, m @ shallow_light(name) + t, e.tris


# ---------------------------------------------------------------------------------------------------------------- reading the trees
def bsp_height(T, mesh=0):
    """Branch levels of mesh `mesh`'s reference-shaped BSP (0: the root is a leaf), walked over Context.mesh_trees()."""
    nodes = T["nodes"]
    root = int(T["meshes"][mesh][0])
    best, stack = 0, [(root, 1)]
    while stack:
        n, level = stack.pop()
        if n < 0:
            continue
        best = max(best, level)
        stack += [(int(nodes["left"][n]), level + 1), (int(nodes["right"][n]), level + 1)]
    return best


def right_spine(T, mesh=0):
    """How many branch nodes the walk passes when it only ever takes the right child: the pending left children of mesh_bsp_narrow."""
    nodes, n, count = T["nodes"], int(T["meshes"][mesh][0]), 0
    while n >= 0:
        count, n = count + 1, int(nodes["right"][n])
    return count


def wide_records(T, mesh=0):
    """child[4] of every two-level record of the mesh (ft_scene.cpp, widen_bsp): RR, RL, LR, LL; [] without a wide root or for a BVH mesh."""
    root, wide_root = int(T["meshes"][mesh][0]), int(T["meshes"][mesh][3])
    if root < 0 or wide_root == INT32_MIN:
        return []
    raw = np.ascontiguousarray(T["nodes"]).view(np.int32).reshape(-1, 16)          # 64-byte units
    out, stack = [], [wide_root]
    while stack:
        u = stack.pop()
        ch = [int(v) for v in raw[u + 4][8:12]]                                     # doubles 36, 37 of the record: unit 4, bytes 32 .. 47
        out.append(ch)
        stack += [c for c in ch if c >= 0]
    return out

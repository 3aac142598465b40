"""Scenes, rays, cameras and CPU-side proofs for tests/test_parallel_rays.py: rays parallel to a flat face, through every cull that
stands in front of the exact intersection.

The rule (Plane.fs:13-16; plane_t in ft_kernels.hip): a ray whose model-space denominator against a flat face has |den| < K_EPS hits
that face at its own origin, t = 0, when the origin is on or above the face and passes the face's clip, however far the origin lies
from the item.  `den` is row . d with `row` a row of the leaf's world-to-model matrix: row 1 for plane, square, circle and
solidCylinder, rows 0, 1 and 2 for the cube.

Everything here is a function of a builder, so that the oracle, a host-only context and the device build the same scene, and the rays
are built from leaf_matrices() of a host-only context: den falls into fixed bands around the rule (K_EPS) and around the culls'
doubled threshold (2 K_EPS).

Faces in model space, as the oracle composes them (Cube.fs:17-25, Cylinder.fs:22-29): `Face(row, offset, sign, clip)` is the plane
model[row] = offset; "above" is sign * (model[row] - offset) > 0; the clip is
    none  the plane: everywhere
    unit  the square: the two other coordinates in [0, 1]
    half  a cube face: the two other coordinates in [-0.5, 0.5]
    ball  the circle (and both caps of the solidCylinder): |hit point - face centre| < 1 - and the hit point of a parallel ray is its
          ORIGIN, so the origin has to lie within the unit BALL around the face's centre, height included (Cylinder.fs:22).
A cube face that looks inward counts as well: flipNormals turns the reported normal, not the plane (the bottom face y = -0.5 is "above"
for every y > -0.5, the right face x = 0.5 for every x < 0.5)."""
import functools
import math
from collections import namedtuple

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from .limit_tools import leaf_colour
from .walk_tools import matrix

K_EPS = 1e-7
SLIGHT_OFFSET = 1e-4                                                # Shading.fs:129
Face = namedtuple("Face", "row offset sign clip")
FACES = {
    "plane": [Face(1, 0.0, +1, "none")],
    "square": [Face(1, 0.0, +1, "unit")],
    "circle": [Face(1, 0.0, +1, "ball")],
    "cube": [Face(1, -0.5, +1, "half"), Face(1, 0.5, +1, "half"), Face(0, -0.5, -1, "half"), Face(0, 0.5, -1, "half"),
             Face(2, -0.5, -1, "half"), Face(2, 0.5, -1, "half")],
    "solidCylinder": [Face(1, 1.0, +1, "ball"), Face(1, 0.0, -1, "ball")],
}
TARGETS = tuple(FACES)
CONTROLS = ("sphere", "cone", "cylinder")                           # no flat face, no direction
MODEL_BOX = {"square": ((0, 0, 0), (1, 0, 1)), "circle": ((-1, 0, -1), (1, 0, 1)), "cube": ((-0.5,) * 3, (0.5,) * 3),
             "solidCylinder": ((-1, 0, -1), (1, 1, 1)), "sphere": ((-1,) * 3, (1,) * 3), "cone": ((-1, 0, -1), (1, 1, 1)),
             "cylinder": ((-1, 0, -1), (1, 1, 1))}                  # ft_scene.cpp, model_box; the plane has none

# den bands: name -> (lo, hi) of |den|.  "zero" and "half" are parallel by the rule; "cull" is not, but lies inside the culls' 2 K_EPS;
# "near" just outside; "far" an ordinary ray (>= 1e-5, and >= 1e-3 |row| so that t = num / den stays well conditioned at |row| = 1e3).
BANDS = {"zero": (0.0, 1e-9), "half": (0.4e-7, 0.6e-7), "cull": (1.3e-7, 1.7e-7), "near": (2.5e-7, 4e-7), "far": (1e-5, np.inf)}
PARALLEL_BANDS = ("zero", "half")

_ROT = ("rotate", (1.0, 2.0, 0.5), 0.7)
_ROT2 = ("rotate", (0.3, -1.0, 0.8), 1.1)
_MOVE = ("translate", (0.4, -0.3, 0.6))
# name -> the transform nodes above the primitive, innermost first
TRANSFORMS = {
    "identity": [],
    "rotate": [[_ROT, _MOVE]],
    "flat": [[("scale", (1.0, 1e-3, 1.0))]],                        # row 1 has length 1e3
    "tall": [[("scale", (1.0, 1e3, 1.0))]],                         # row 1 has length 1e-3: a thousand times the band of directions
    "shear": [[_ROT, ("scale", (1.3, 0.6, 0.9)), _ROT2, _MOVE]],
    "mirror": [[("scale", (-1.0, 1.0, 1.0))]],
    "nested": [[_ROT, ("scale", (1.3, 0.6, 0.9))], [_ROT2, _MOVE]],  # `shear` split over two nodes
}
STRUCTURES = ("bare", "subA", "intA", "subB", "intB")
TARGET_LEAF = {"bare": 0, "subA": 0, "intA": 0, "subB": 1, "intB": 1, "nine": 0, "three": 0, "many": 0}
ITEM_LEAVES = {"nine": 3, "three": 3}                               # leaves whose boxes bound the target's item (default: the target alone)
_CUBE_TURNS = [((1.0, 0.3 * k, 0.2 + 0.1 * k), 0.35 + 0.23 * k) for k in range(12)]   # twelve distinct rotations: 36 distinct directions


def flat_ops(xf):
    return [op for node in TRANSFORMS[xf] for op in node]


def _under(b, node, xf):
    for ops in TRANSFORMS[xf]:
        node = b.transform(list(ops), node)
    return node


def _control(b, k, centre, size=0.7):
    n = b.transform([("scale", size), ("rotate", (0.2, 1.0, -0.4), 0.5 + k), ("translate", tuple(float(v) for v in centre))], b.primitive(H.PRIMS[CONTROLS[k]]))
    return b.material(n, colour=leaf_colour(10 + k), shineyness=4.0)


def build_scene(b, prim, xf, structure="bare", controls=None, size=0.7, lights=(), reach=4.0):
    """The target (leaf TARGET_LEAF[structure]) as the first top-level item, then - with `controls`, three world-space centres - a
    sphere, a cone and a cylinder.  Structures: bare; subA: target - S with a small sphere S cutting into it; intA: target & S with S a
    sphere of radius `reach` about the target's origin, large enough to hold every ray origin (an origin hit of A survives an
    intersection only inside B; under a closed A the item's bounds are still A's alone); subB / intB: S - target and S & target with S a sphere of radius 1.5 about the target's origin (B's bounds are dropped, its
    directions count); nine: a union of three differently rotated cubes under `xf`, one item with 9 directions; three: the same union
    with one rotation for all three, 3 directions; many: twelve differently rotated cubes, 36 directions.
    lights: ("directional", dir, colour) | ("point", pos, colour)."""
    b.clear()
    m, t = matrix(flat_ops(xf))
    if structure in ("nine", "three", "many"):
        n_cubes = 12 if structure == "many" else 3
        turn = lambda k: _CUBE_TURNS[0 if structure == "three" else k]
        step = {"nine": 0.0, "three": 0.3, "many": 1.7}[structure]
        cubes = [b.material(b.transform([("rotate",) + turn(k), ("translate", (step * k, 0.0, 0.0))], b.primitive(ft.CUBE)), colour=leaf_colour(k)) for k in range(n_cubes)]
        items = [_under(b, b.union(b.union(cubes[0], cubes[1]), cubes[2]), xf)] if n_cubes == 3 else [_under(b, c, xf) for c in cubes]
    else:
        tgt = b.material(_under(b, b.primitive(H.PRIMS[prim]), xf), colour=leaf_colour(TARGET_LEAF[structure]), shineyness=4.0)   # a hit's colour names its leaf
        if structure == "bare":
            items = [tgt]
        else:
            is_a = structure.endswith("A")
            c = m @ np.array([0.2, 0.1, 0.2]) + t if structure == "subA" else t
            radius = {"subA": 0.4, "intA": reach}.get(structure, 1.5)
            s = b.material(b.transform([("scale", radius), ("translate", tuple(c))], b.primitive(ft.SPHERE)), colour=leaf_colour(1 if is_a else 0))
            op = ft.SUBTRACT if structure.startswith("sub") else ft.INTERSECT
            items = [b.csg(op, tgt, s) if is_a else b.csg(op, s, tgt)]
    if controls is not None:
        items += [_control(b, k, c, size) for k, c in enumerate(controls)]
    b.set_objects(b.group(items))
    for kind, v, colour in lights:
        if kind == "directional":
            b.add_directional(tuple(v), tuple(colour))
        else:
            b.add_positional(tuple(v), (1.0, 0.0, 0.0), tuple(colour))
    b.commit()


def host_facts(build, *args, **kw):
    """(scene_info, m2w, w2m) of a scene on a host-only context."""
    ctx = ft.Context(host_only=True)
    build(ctx, *args, **kw)
    info = ctx.scene_info()
    m2w, w2m = ctx.leaf_matrices()
    ctx.close()
    return info, m2w, w2m


def bounding_sphere(prim, m2w):
    """Centre and radius of the target's item as Flattener::end_item finds them: the eight transformed corners of the model box (of
    every leaf, when m2w holds several), the middle of their bounds, the furthest corner.  None for the plane."""
    if prim == "plane":
        return None
    lo, hi = MODEL_BOX[prim]
    corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)], dtype=np.float64)
    pts = np.concatenate([corners @ M[:, :3].T + M[:, 3] for M in np.asarray(m2w).reshape(-1, 3, 4)])
    centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    return centre, float(np.linalg.norm(pts - centre, axis=1).max())


def union_sphere(leaves):
    """The same over several (primitive, m2w) leaves: the bounds of an item whose operands all count."""
    pts = []
    for prim, M in leaves:
        lo, hi = MODEL_BOX[prim]
        corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)], dtype=np.float64)
        pts.append(corners @ M[:, :3].T + M[:, 3])
    pts = np.concatenate(pts)
    centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    return centre, float(np.linalg.norm(pts - centre, axis=1).max())


def line_distance(o, d, c):
    w = c - o
    along = np.einsum("ij,ij->i", w, d) / np.einsum("ij,ij->i", d, d)
    return np.linalg.norm(w - along[:, None] * d, axis=1)


def cone_clearance(apex, spread, dirs, centre):
    """How far `centre` lies outside the cone with the given apex (origins within `spread` of it), the mean of `dirs` as its axis and
    their largest deviation as its half-angle; <= 0: inside."""
    u = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    a = u.mean(axis=0); a /= np.linalg.norm(a)
    theta = float(np.arccos(np.clip(u @ a, -1.0, 1.0)).max())
    v = centre - apex
    psi = math.acos(float(np.clip(v @ a / np.linalg.norm(v), -1.0, 1.0)))
    gap = psi - theta
    dist = np.linalg.norm(v) * (math.sin(gap) if gap < math.pi / 2 else 1.0)
    return (dist if gap > 0 else 0.0) - spread


# ---------------------------------------------------------------------------------------------------------------- model space
def _inside(face, p):
    others = [a for a in range(3) if a != face.row]
    if face.clip == "none":
        return True, np.inf
    if face.clip == "ball":
        q = np.array(p, dtype=np.float64); q[face.row] -= face.offset
        return np.linalg.norm(q) < 1.0, abs(np.linalg.norm(q) - 1.0)
    lo, hi = (0.0, 1.0) if face.clip == "unit" else (-0.5, 0.5)
    margin = min(min(abs(p[a] - lo), abs(p[a] - hi)) for a in others)
    return all(lo <= p[a] <= hi for a in others), margin


def origin_hit_expected(prim, row, p):
    """Does a ray from model point p, parallel to the faces of `row`, hit one of them at its origin?"""
    return any(f.sign * (p[row] - f.offset) > 0 and _inside(f, p)[0] for f in FACES[prim] if f.row == row)


def model_origins(prim, row, c_axis, far):
    """Model-space origins for the faces of `row`: heights of 1e-3 and 0.3 (1e-3 .. 0.99 under a ball clip) on both sides of every face and
    `far`, 1.7 `far` and 2.5 `far` on both sides of the item's centre (c_axis, its coordinate along the row), each over clip coordinates at least
    1e-3 inside and outside the clip.  Points closer than 1e-3 to a face plane or a clip boundary are left out."""
    faces = [f for f in FACES[prim] if f.row == row]
    clip = faces[0].clip
    axis = {c_axis + s * far for s in (-2.5, -1.7, -1.0, 1.0, 1.7, 2.5)}
    for f in faces:
        for h in ((1e-3, 0.3, 0.7, 0.9, 0.99) if clip == "ball" else (1e-3, 0.3)):
            axis |= {f.offset + h, f.offset - h}
    if clip == "none":
        uv = [(0.5, 0.5), (-40.0, 13.0), (7.0, 7.0)]
    elif clip == "ball":
        uv = [(0.0, 0.0), (0.01, 0.02), (0.05, -0.1), (0.6, -0.7), (0.9, 0.3), (1.2, 0.1), (5.0, 5.0)]
    else:
        uv = [(0.5, 0.5), (0.001, 0.6), (0.999, 0.3), (0.4, 0.999), (-0.001, 0.5), (1.001, 0.5), (0.5, -0.4), (6.0, 0.5)]
        if clip == "half":
            uv = [(u - 0.5, v - 0.5) for u, v in uv]
    others = [a for a in range(3) if a != row]
    out = []
    for h in sorted(axis):
        for u, v in uv:
            p = np.zeros(3); p[row] = h; p[others[0]] = u; p[others[1]] = v
            if all(abs(h - f.offset) >= 1e-3 and _inside(f, p)[1] >= 1e-3 for f in faces):
                out.append(p)
    return np.array(out)


def in_plane_basis(R):
    n = R / np.linalg.norm(R)
    e1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.7 else [0.0, 1.0, 0.0]); e1 /= np.linalg.norm(e1)
    return n, e1, np.cross(n, e1)


def band_den(rng, band, R_len):
    if band == "zero":
        return float(rng.choice([0.0, 5e-10]))
    if band == "far":
        return max(1e-5, 1e-3 * R_len) * 10.0 ** rng.uniform(0.0, 2.0)
    lo, hi = BANDS[band]
    return rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))


Rays = namedtuple("Rays", "o d row band den model expected far max_dist")


def case_rays(prim, xf, structure, m2w, w2m, per_point=2, seed=0):
    """The explicit rays of a case, for every face row of the target leaf: every model origin x band x sign of den x `per_point`
    directions in the face's plane plus den / |row|^2 row.  On the unbounded plane a ray of the three non-parallel bands would meet it
    at t = num / den ~ 1e4 .. 1e7 with den known to nine digits at best, so there den takes the sign that puts the crossing behind
    the origin (both signs still occur: the origins lie on both sides).  Rays whose line passes the item's bounding sphere by more than
    two radii come first, a multiple of 64 of them: whole waves that no lane's bounding-sphere test keeps."""
    leaf = TARGET_LEAF[structure]
    M, W = m2w[leaf], w2m[leaf]
    sphere = bounding_sphere(prim, m2w[leaf:leaf + ITEM_LEAVES.get(structure, 1)])
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in Rays._fields}
    rows = sorted({f.row for f in FACES[prim]})
    for row in rows:
        R = W[row, :3]
        R_len = float(np.linalg.norm(R))
        n, e1, e2 = in_plane_basis(R)
        if sphere is None:
            c_axis, far = 0.0, 50.0
        else:
            c_axis, far = float(R @ sphere[0] + W[row, 3]), 3.0 * sphere[1] * R_len
        for p in model_origins(prim, row, c_axis, far):
            o = M[:, :3] @ p + M[:, 3]
            height_sign = 1.0 if p[row] > 0 else -1.0
            for band in BANDS:
                for sign in (1.0, -1.0):
                    if prim == "plane" and band not in PARALLEL_BANDS:
                        sign = height_sign
                    for _ in range(per_point):
                        den = sign * band_den(rng, band, R_len)
                        while True:                                 # an ordinary ray for the leaf's other rows
                            phi, s = rng.uniform(0, 2 * math.pi), rng.uniform(0.3, 3.0)
                            d = s * (math.cos(phi) * e1 + math.sin(phi) * e2) + (den / (R_len * R_len)) * R
                            if all(abs(W[other, :3] @ d) >= 2e-5 for other in rows if other != row):
                                break
                        cols["o"].append(o); cols["d"].append(d); cols["row"].append(row); cols["band"].append(band)
                        cols["den"].append(float(R @ d)); cols["model"].append(p)
                        cols["expected"].append(band in PARALLEL_BANDS and origin_hit_expected(prim, row, p))
                        cols["max_dist"].append(rng.uniform(0.5, 5.0))
    o, d = np.array(cols["o"]), np.array(cols["d"])
    far = np.zeros(len(o), bool) if sphere is None else line_distance(o, d, sphere[0]) > 2.0 * sphere[1]
    order = np.argsort(~far, kind="stable")
    n_far = int(far.sum()) // 64 * 64                               # (the far rays beyond the last whole wave stay far; they just share a wave)
    out = Rays(o[order], d[order], np.array(cols["row"])[order], np.array(cols["band"])[order], np.array(cols["den"])[order],
               np.array(cols["model"])[order], np.array(cols["expected"])[order], far[order], np.array(cols["max_dist"])[order])
    return out, sphere, n_far


def control_centres(rays, sphere):
    """Three world points ON far origin-hit rays (1.5 d from their origins): the controls stand in the way of the very rays that hit
    the target at their origin, and must not be hit at t = 0 themselves."""
    pick = np.nonzero(rays.expected & rays.far)[0]
    if len(pick) == 0:
        pick = np.nonzero(rays.expected)[0]
    pick = pick[[0, len(pick) // 2, len(pick) - 1]]
    return [rays.o[k] + 1.5 * rays.d[k] for k in pick]


def leaf_of_colour(col, hit):
    """The leaf a hit's material colour names (limit_tools.leaf_colour; controls are 10, 11, 12); -1 for a miss."""
    out = np.full(len(col), -1, dtype=np.int64)
    for i in list(range(12)) + [10, 11, 12]:
        out[(np.abs(col - np.array(leaf_colour(i))).max(axis=1) < 1e-12) & hit.astype(bool)] = i
    return out


CLOSED = ("cube", "solidCylinder")                                  # ft_scene.cpp, closed_solid: under such an A, operand B does not widen the item's bounds


@functools.lru_cache(maxsize=None)
def reference(prim, xf, structure, alone=False):
    """One explicit-ray case, built and answered once: facts of a host-only context, the rays, and the oracle's closest / blocked."""
    probe = host_facts(build_scene, prim, xf, structure)
    rays, sphere, n_far = case_rays(prim, xf, structure, probe[1], probe[2])
    controls = None if alone else control_centres(rays, sphere)
    reach = 1.2 * float(np.linalg.norm(rays.o - matrix(flat_ops(xf))[1], axis=1).max())          # intA: its sphere holds every origin
    info, m2w, w2m = host_facts(build_scene, prim, xf, structure, controls, reach=reach)
    orc = O.Oracle()
    build_scene(orc, prim, xf, structure, controls, reach=reach)
    closest = orc.closest(rays.o, rays.d)
    blocked = orc.blocked(rays.o, rays.d, rays.max_dist)
    orc.close()
    for a in tuple(rays) + tuple(closest) + (blocked,):
        a.setflags(write=False)
    return {"info": info, "m2w": m2w, "w2m": w2m, "rays": rays, "sphere": sphere, "n_far": n_far, "controls": controls, "reach": reach, "closest": closest,
            "blocked": blocked, "leaf": TARGET_LEAF[structure]}


def origin_hits(ref):
    """Rays the oracle answers with t == 0 on the target leaf."""
    hit, t, _, _, col = ref["closest"]
    return (hit != 0) & (t == 0.0) & (leaf_of_colour(col, hit) == ref["leaf"])


# ---------------------------------------------------------------------------------------------------------------- frames
View = namedtuple("View", "name eye look up fov w h tiles spp jitter py")


def camera(view):
    return ft.make_camera(tuple(view.eye), tuple(view.look), tuple(view.up), view.fov, view.w / view.h)


def row_view(name, R, eye, w, h, py, den=0.0, fov=math.radians(40.0), spin=0.4, tiles=None, spp=1, jitter=None, sample=0):
    """A pinhole view whose pixel row `py` (sample `sample` of the jitter pattern) sends every ray at row . d = den: the camera's i lies
    in the face's plane, its up vector is the face's normal, and k is tilted out of the plane by the angle that cancels the row's own
    elevation.  With pixel height = height / (res_h - 1) (sic, Image.fs:71) no row of a 72- or 61-wide frame is level by itself."""
    jitter = np.zeros((1, 2)) if jitter is None else np.asarray(jitter, dtype=np.float64)
    n, e1, e2 = in_plane_basis(np.asarray(R, dtype=np.float64))
    i0 = math.cos(spin) * e1 + math.sin(spin) * e2
    m = np.cross(i0, n)                                             # n x m = i0
    ip = O.image_plane(ft.make_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), fov, w / h), w, h)
    jy = ip["top_left"][1] - py * ip["pixel_height"] + jitter[sample, 1] * ip["pixel_height"]
    alpha = math.asin((den / np.linalg.norm(R)) / math.sqrt(1.0 + jy * jy)) - math.atan(jy)
    k = math.cos(alpha) * m + math.sin(alpha) * n
    return View(name, np.asarray(eye, dtype=np.float64), np.asarray(eye) + k, n, fov, w, h, tiles, spp, jitter, py)


def pixels_of(view):
    if view.tiles is None:
        return [(x, y) for y in range(view.h) for x in range(view.w)]
    return sorted({(x, y) for (x0, y0, tw, th) in view.tiles for y in range(max(0, y0), min(view.h, y0 + th)) for x in range(max(0, x0), min(view.w, x0 + tw))},
                  key=lambda p: (p[1], p[0]))


def pixel_rays(view, sample=0):
    """The geometry rays of the view's tile pixels for one sample of its jitter pattern, from the oracle's ray_through_pixel: origins
    (before slightOffset), directions, xs, ys."""
    cam, px = camera(view), pixels_of(view)
    o, d = np.zeros((len(px), 3)), np.zeros((len(px), 3))
    for k, (x, y) in enumerate(px):
        o[k], d[k] = O.ray_through_pixel(cam, view.w, view.h, x, y, float(view.jitter[sample, 0]), float(view.jitter[sample, 1]))
    return o, d, np.array([p[0] for p in px]), np.array([p[1] for p in px])


def view_controls(view, distance, share=0.3):
    """Three centres in front of the eye, spread over the frame, and a size: `share` of the frame's half height.  (Under the 0.05
    degree views the controls are large, 1.5: a sphere 7700 radii away, as a share of 0.3 would have it, is met through a quadratic
    whose discriminant cancels nine digits, and the normals of grazing hits then differ by more than helpers.assert_hits_match allows
    between any two orders of the same arithmetic.)"""
    cam_k = (view.look - view.eye) / np.linalg.norm(view.look - view.eye)
    i = np.cross(view.up, cam_k); i /= np.linalg.norm(i)
    j = np.cross(cam_k, i)
    half = math.tan(view.fov / 2.0)
    centres = [view.eye + distance * (cam_k + fx * half * (view.w / view.h) * i + fy * half * j) for fx, fy in ((-0.55, 0.35), (0.05, -0.3), (0.6, 0.2))]
    return centres, share * distance * half


def waves_of(view):
    """({(x, y): wave}, tiled) as list_pixels (ft_frame.cpp) lays the frame's pixels out: a rect whose sides are multiples of 8 goes in
    8 x 8 blocks from its own corner, any other row by row, and a wave takes 64 consecutive pixels of the list.  tiled: every rect
    is made of blocks - only then does k_classify run."""
    rects = [(0, 0, view.w, view.h)] if view.tiles is None else view.tiles
    order, tiled = [], True
    for x0, y0, w, h in rects:
        x0, y0, w, h = max(x0, 0), max(y0, 0), min(x0 + w, view.w) - max(x0, 0), min(y0 + h, view.h) - max(y0, 0)
        if w % 8 == 0 and h % 8 == 0:
            order += [(x0 + tx + ix, y0 + ty + iy) for ty in range(0, h, 8) for tx in range(0, w, 8) for iy in range(8) for ix in range(8)]
        else:
            tiled = False
            order += [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    return {p: k // 64 for k, p in enumerate(order)}, tiled


def wave_clearances(view, pixels, centre, extent=1.0):
    """For each wave that holds one of `pixels` (x, y): how far `centre` lies outside the cone around the rays of all its pixels, each
    pixel grown by `extent` pixels on every side (the classifier grows a block by the jitter pattern's reach, at least one pixel)."""
    cam = camera(view)
    waves, _ = waves_of(view)
    out = {}
    for key in {waves[p] for p in pixels}:
        members = [p for p, w in waves.items() if w == key]
        dirs = np.array([O.ray_through_pixel(cam, view.w, view.h, x, y, jx, jy)[1] for x, y in members
                         for jx in (-0.5 - extent, 0.5 + extent) for jy in (-0.5 - extent, 0.5 + extent)])
        out[key] = cone_clearance(view.eye, 0.0, dirs, centre)
    return out


FRAME_LIGHTS = (("directional", (-0.4, -1.0, 0.6), (1.0, 0.9, 0.8)), ("point", (30.0, 40.0, -50.0), (0.3, 0.35, 0.5)))

# prim, transform: the frames' targets.  The circle and the solidCylinder only under `tall`: their clip is a unit ball around the face's
# centre, which no origin outside the item's bounding sphere reaches unless the transform stretches the ball past the sphere.
# "nine": the union of three differently rotated cubes, whose item has no OP_CULL of its own.
FRAME_CASES = [("square", "rotate"), ("square", "flat"), ("cube", "shear"), ("cube", "mirror"), ("cube", "nested"), ("cube", "tall"),
               ("circle", "tall"), ("solidCylinder", "tall"), ("plane", "rotate"), ("nine", "rotate")]
FRAME_KINDS = ("level", "band", "tiles", "jitter")


def frame_target(prim):
    """(primitive, structure, leaves of the target's item) of a frame case."""
    return ("cube", "nine", 3) if prim == "nine" else (prim, "bare", 1)


def frame_eye(prim, xf, m2w, w2m, row=1, n_leaves=1):
    """A model point inside the clip of a face of `row`, above it, three bounding radii from the item's centre along the face's normal
    (0.99 above the face under a ball clip; 50 above the plane), in world space."""
    M, W = m2w[0], w2m[0]
    sphere = bounding_sphere(prim, m2w[:n_leaves])
    R_len = float(np.linalg.norm(W[row, :3]))
    f = FACES[prim][0]
    others = [a for a in range(3) if a != row]
    p = np.zeros(3)
    p[others[0]], p[others[1]] = {"none": (0.5, 0.5), "unit": (0.3, 0.6), "half": (-0.2, 0.1), "ball": (0.01, 0.02)}[f.clip]
    if f.clip == "ball":
        p[row] = f.offset + f.sign * 0.99
    elif sphere is None:
        p[row] = 50.0
    else:
        p[row] = float(W[row, :3] @ sphere[0] + W[row, 3]) + f.sign * 3.0 * sphere[1] * R_len
    assert origin_hit_expected(prim, row, p)
    return M[:, :3] @ p + M[:, 3], sphere


@functools.lru_cache(maxsize=None)
def frame_reference(prim, xf, kind):
    """One frame case on the oracle: the view, the scene's controls, sample 0's rays and their closest hits, and the frame.
    level: row py of a 72 x 33 frame at den = 0.  band: the same row at den = 1.5e-7 (looking away from the face on the plane, so that
    the crossing lies behind the eye).  tiles: 61 x 37 under a list of two tiles.  jitter: spp 2 under jitter_pattern(2), sample 0 of the
    row parallel, one tile of 72 x 32.  Neither 72 x 33 nor 61 x 37 is made of 8 x 8 blocks, and k_classify only runs on pixel lists that
    are: the two tile lists are what brings it in.  Under `tall` the field of view is 0.05 degrees: rows are 1.2e-5 apart, |row| = 1e-3, and nine rows fall under K_EPS."""
    prim, structure, n_leaves = frame_target(prim)
    _, m2w, w2m = host_facts(build_scene, prim, xf, structure)
    R = w2m[0][1, :3]
    eye, sphere = frame_eye(prim, xf, m2w, w2m, n_leaves=n_leaves)
    fov = math.radians(0.05 if xf == "tall" else 12.0)
    w, h, py = (72, 33, 19) if kind != "tiles" else (61, 37, 20)
    tiles = {"tiles": [(0, 0, 24, 32), (24, 5, 32, 24)], "jitter": [(0, 0, 72, 32)]}.get(kind)   # sides in multiples of 8: these frames are classified
    jitter = ft.jitter_pattern(2) if kind == "jitter" else None
    view = row_view(kind, R, eye, w, h, py, den=1.5e-7 if kind == "band" else 0.0, fov=fov, tiles=tiles, spp=2 if kind == "jitter" else 1, jitter=jitter)
    controls, size = view_controls(view, 2000.0 if xf == "tall" else 9.0, 1.5 if xf == "tall" else 0.3)
    orc = O.Oracle()
    build_scene(orc, prim, xf, structure, controls, size, FRAME_LIGHTS)
    o, d, xs, ys = pixel_rays(view)
    closest = orc.closest(o + SLIGHT_OFFSET * d, d)
    frame, stats = orc.render(camera(view), view.w, view.h, view.spp, view.jitter, tiles=view.tiles, seed=ft.DEFAULT_SEED)
    orc.close()
    for a in (o, d, xs, ys, frame) + tuple(closest):
        a.setflags(write=False)
    return {"view": view, "controls": controls, "size": size, "o": o, "d": d, "xs": xs, "ys": ys, "closest": closest, "frame": frame, "stats": stats,
            "R": R, "sphere": sphere}


def build_frame_scene(b, prim, xf, ref):
    prim, structure, _ = frame_target(prim)
    build_scene(b, prim, xf, structure, ref["controls"], ref["size"], FRAME_LIGHTS)


# ---------------------------------------------------------------------------------------------------------------- shadows
# An occluder cube under `rotate`, a receiver sphere of radius 1.5 eight model units above it (it reaches into the clip prism of the cube's
# bottom face, which looks up the whole column), a cone beside it.  directional: the light's direction lies in the cube's y faces, so every
# shadow ray is parallel to them, and the receiver's points inside the column |x|, |z| < 0.5 are blocked at t = 0.  point: the light
# stands in the plane through the eye that holds pixel row `py` - that plane is level with the faces - so the shadow rays of that one
# row are parallel, and the column draws a dark dash on one pixel row.
SHADOW_XF = "rotate"
SHADOW_KINDS = ("directional", "point")
BALL_AT = (1.2, 8.0, 0.3)                                           # (model space of the cube) its equator crosses the column at (-0.3, 8, 0.3)


def _shadow_layout():
    _, m2w, w2m = host_facts(build_scene, "cube", SHADOW_XF)
    M, W = m2w[0], w2m[0]
    to_world = lambda p: M[:, :3] @ np.asarray(p, dtype=np.float64) + M[:, 3]
    return M, W, to_world


def build_shadow_scene(b, kind, light):
    _, _, to_world = _shadow_layout()
    b.clear()
    cube = b.material(_under(b, b.primitive(ft.CUBE), SHADOW_XF), colour=leaf_colour(0))
    ball = b.material(b.transform([("scale", 1.5), ("translate", tuple(to_world(BALL_AT)))], b.primitive(ft.SPHERE)), colour=leaf_colour(1), shineyness=4.0)
    cone = b.material(b.transform([("scale", 0.8), ("translate", tuple(to_world((-1.6, 7.2, -2.2))))], b.primitive(ft.CONE)), colour=leaf_colour(2))
    b.set_objects(b.group([cube, ball, cone]))
    if kind == "directional":
        b.add_directional(tuple(light), (1.0, 0.9, 0.8))
    else:
        b.add_positional(tuple(light), (1.0, 0.0, 0.0), (1.0, 0.9, 0.8))
    b.commit()


@functools.lru_cache(maxsize=None)
def shadow_reference(kind):
    M, W, to_world = _shadow_layout()
    R = W[1, :3]
    eye = to_world((-4.0, 8.0, -5.0))
    # aim the view at the receiver: spin the in-plane frame until k points at it (the row stays level whatever the spin)
    aim = to_world((0.3, 8.0, 0.0)) - eye
    best = min(np.linspace(0.0, 2 * math.pi, 721), key=lambda s: -float((row_view(kind, R, eye, 72, 33, 14, fov=math.radians(20.0), spin=s).look - eye) @ aim))
    view = row_view(kind, R, eye, 72, 33, 14, fov=math.radians(20.0), spin=float(best))
    if kind == "directional":
        light_arg = M[:, :3] @ np.array([0.6, 0.0, 0.8])            # shining along model (0.6, 0, 0.8): in the y faces
    else:
        light_arg = to_world((-5.0, 8.0, 2.0))
    orc = O.Oracle()
    build_shadow_scene(orc, kind, light_arg)
    o, d, xs, ys = pixel_rays(view)
    closest = orc.closest(o + SLIGHT_OFFSET * d, d)
    m = closest[0].astype(bool)
    p = closest[2][m]
    so = p + SLIGHT_OFFSET * closest[3][m]                          # getLightsOnPoint, Shading.fs:109-117: off the surface along the normal
    if kind == "directional":
        sd = np.tile(-light_arg, (len(p), 1))                       # Shading.fs:35-37: not normalised
        dist = np.full(len(p), np.finfo(np.float64).max)
    else:
        sd = light_arg - so                                         # Shading.fs:38-42: from the offset point
        dist = np.linalg.norm(sd, axis=1)
        sd = sd / dist[:, None]
    blocked = orc.blocked(so, sd, dist)
    frame, stats = orc.render(camera(view), view.w, view.h, 1, np.zeros((1, 2)), seed=ft.DEFAULT_SEED)
    orc.close()
    return {"view": view, "light": light_arg, "R": R, "W": W, "so": so, "sd": sd, "dist": dist, "blocked": blocked, "xs": xs[m], "ys": ys[m],
            "frame": frame, "stats": stats, "sphere": bounding_sphere("cube", M), "hit_leaf": leaf_of_colour(closest[4], closest[0])[m]}


# ---------------------------------------------------------------------------------------------------------------- reflections
# A mirror y = 3 seen from (0, 1, -6) along +z (every row of a 72 x 33 frame looks up: Image.fs:71 again): pixel row py climbs at slope s
# and its rays leave the mirror as (x, -s, 1).  A cube turned about x until its y faces have the normal (0, 1, s) / |.| is parallel to
# every one of those, and it stands twelve units down its own normal from the line where the row meets the mirror, six wide in x: the
# reflections of the pixels with |x| < 3 start inside the column above its bottom face and hit it at t = 0.
MIRROR_PY = 24
MIRROR_Y = 3.0


def mirror_layout(w=72, h=33):
    eye = np.array([0.0, 1.0, -6.0])
    view = View("mirror", eye, eye + np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0]), math.radians(40.0), w, h, None, 1, np.zeros((1, 2)), MIRROR_PY)
    _, d = O.ray_through_pixel(camera(view), w, h, 0, MIRROR_PY, 0.0, 0.0)
    s = d[1] / d[2]
    angle = math.atan(s)
    z1 = eye[2] + (MIRROR_Y - eye[1]) / s                           # where the row meets the mirror
    normal = np.array([0.0, math.cos(angle), math.sin(angle)])
    centre = np.array([0.0, MIRROR_Y, z1]) - 12.0 * normal
    return view, s, angle, centre


def build_mirror_scene(b):
    view, s, angle, centre = mirror_layout()
    b.clear()
    mirror = b.material(b.translate((0.0, MIRROR_Y, 0.0), b.primitive(ft.PLANE)), colour=(0.9, 0.9, 0.9), reflectance=0.8)
    cube = b.material(b.transform([("scale", (6.0, 1.0, 1.0)), ("rotate", (1.0, 0.0, 0.0), angle), ("translate", tuple(centre))], b.primitive(ft.CUBE)), colour=leaf_colour(1), shineyness=4.0)
    ball = b.material(b.transform([("scale", 0.8), ("translate", (2.0, 2.2, 4.0))], b.primitive(ft.SPHERE)), colour=leaf_colour(2), reflectance=0.3)
    cone = b.material(b.transform([("scale", 0.9), ("translate", (-2.2, 1.4, 5.0))], b.primitive(ft.CONE)), colour=leaf_colour(3))
    b.set_objects(b.group([mirror, cube, ball, cone]))
    b.add_directional((-0.4, -1.0, 0.6), (1.0, 0.9, 0.8))
    b.commit()

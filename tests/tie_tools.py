"""An exact reference for hit selection and CSG, and the rays and scenes of tests/test_exact_ties.py.

The reference is a restatement of the F# text over fractions.Fraction: the primitives in their own model frame (Sphere.fs:11-21,
Plane.fs:9-20, Cube.fs:9-25, Cone.fs:7-27, Cylinder.fs:8-29, Math.fs:4-10), Csg.fs:19-94, Scene.fs:112-121.  It shares nothing with
the oracle or the device.  Two things are evaluated as the geometry they stand for and not through the reference's rotation
matrices: the cube's side faces and the solidCylinder's bottom cap are exact squares and an exact circle (the device
carries no cos 90 / sin 180 residues); comparisons made there are tagged `residue`, and a ray on which one of them is an equality is a
residue ray: on it the F# program is decided by a 6e-17 residue and the oracle is not the expectation.

Every comparison the reference makes goes through a `Cmps` list, so that a ray can be judged afterwards (`robust`): it is kept only if
each comparison is an equality of exactly representable doubles or is decided by a margin of 1e-9.

Trees are those of tests/limit_tools.py, with transforms only in a primitive's own `ops`:
    ("prim", kind, ops, i)   ("group", [tree, ...])   ("csg", op, A, B)
"""
import math
from collections import namedtuple
from fractions import Fraction as F

import numpy as np

import functracer_amd as ft

from . import helpers as H
from .limit_tools import build_tree, leaf_colour, tree_facts  # noqa: F401  (re-exported for the tests)

OPS = {"union": ft.UNION, "intersect": ft.INTERSECT, "subtract": ft.SUBTRACT, "exclude": ft.EXCLUDE}
KIND_NAME = {v: k for k, v in H.PRIMS.items()}
MARGIN = F(1, 10 ** 9)

Hit = namedtuple("Hit", "t leaf sub flip n res key")  # n: the world normal as floats; res: from a residue face; key: (kind, ops, sub), None if unknown


class Irrational(Exception):
    """A degenerate quadratic (a = 0: the reference divides by zero): the ray leaves the exact families."""


class Cmps(list):
    """The comparisons made for one ray: (a, b, equality is decidable in doubles, values that must be exact for that, residue)."""

    def rec(self, a, b, eq_ok=True, deps=(), residue=False):
        self.append((a, b, eq_ok, deps, residue))

    def lt(self, a, b, **kw):
        self.rec(a, b, **kw)
        return a < b

    def le(self, a, b, **kw):
        self.rec(a, b, **kw)
        return a <= b

    def ge(self, a, b, **kw):
        self.rec(a, b, **kw)
        return a >= b


def is_small_dyadic(x):
    """Exactly representable in binary64 with room to spare: sums and products of a few such values are exact too."""
    x = F(x)
    d = x.denominator
    return d & (d - 1) == 0 and d <= 2 ** 30 and abs(x.numerator).bit_length() <= 30


def robust(cmps):
    """The keeping rule: every comparison is an equality of exact doubles, or decided by 1e-9 relative (to max(1, |a|, |b|): several of
    them are against 0)."""
    for a, b, eq_ok, deps, _ in cmps:
        if a == b:
            if not (eq_ok and is_small_dyadic(a) and is_small_dyadic(b) and all(is_small_dyadic(v) for v in deps)):
                return False
        elif abs(a - b) < MARGIN * max(1, abs(a), abs(b)):
            return False
    return True


def has_residue_equality(cmps):
    return any(res and a == b for a, b, _, _, res in cmps)


def fsqrt(x):
    """The exact root of a rational square; of anything else the root to 30 decimals.  Such a value is no small dyadic, so `robust`
    drops every ray on which it meets an equality, and every other kept comparison has a margin of 1e-9: the verdicts are those of
    exact arithmetic."""
    assert x >= 0
    n, d = math.isqrt(x.numerator), math.isqrt(x.denominator)
    if n * n == x.numerator and d * d == x.denominator:
        return F(n, d)
    return F(math.isqrt(x.numerator * 10 ** 60 // x.denominator), 10 ** 30)


# ---- the primitives in their model frame: lists of (t, sub, model normal) in the order of the text --------------------------------

EPS = F(1, 10 ** 7)                                               # Plane.fs:11


def _plane_t(num, den, C, residue=False):
    """Plane.fs:12-20 with num = (p0 - o).n and den = d.n; None when the sequence is empty."""
    if C.lt(abs(den), EPS, residue=residue):
        return F(0) if C.lt(num, EPS, residue=residue) else None
    return num / den


def _unit(v):
    """normalise (CommonTypes.fs:63-67): a vector shorter than 1e-7 is returned as it is (the cone's apex: the zero vector)."""
    x, y, z = (float(c) for c in v)
    l = math.sqrt(x * x + y * y + z * z)
    return (x, y, z) if l < 1e-7 else (x / l, y / l, z / l)


def _in_square(u, v, t, C, residue=False):
    kw = dict(deps=(t,), residue=residue)
    return C.ge(u, 0, **kw) and C.le(u, 1, **kw) and C.ge(v, 0, **kw) and C.le(v, 1, **kw)


def _in_circle(x, z, t, C, residue=False):
    return C.lt(x * x + z * z, 1, deps=(t,), residue=residue)   # |p| < 1 as |p|^2 < 1: the same verdict, the margin on |p|^2 is the wider


def plane(o, d, C):
    t = _plane_t(-o[1], d[1], C)
    return [] if t is None else [(t, 0, (0.0, 1.0, 0.0))]


def square(o, d, C):
    t = _plane_t(-o[1], d[1], C)
    if t is None or not _in_square(o[0] + t * d[0], o[2] + t * d[2], t, C):
        return []
    return [(t, 0, (0.0, 1.0, 0.0))]


def circle(o, d, C):
    t = _plane_t(-o[1], d[1], C)
    if t is None or not _in_circle(o[0] + t * d[0], o[2] + t * d[2], t, C):
        return []
    return [(t, 0, (0.0, 1.0, 0.0))]


def cube(o, d, C):
    """Cube.fs:17-25: bottom, top, left, right, front, back in the [0, 1]^3 frame behind translate (-.5, -.5, -.5).  left is the square
    rotated 90 degrees about z (local frame (y, -x, z)), front the square rotated -90 degrees about x (local frame (x, -z, y))."""
    q = (o[0] + F(1, 2), o[1] + F(1, 2), o[2] + F(1, 2))
    out = []
    faces = [(-q[1], d[1], 0, 2, (0.0, -1.0, 0.0), False), (-(q[1] - 1), d[1], 0, 2, (0.0, 1.0, 0.0), False),
             (q[0], -d[0], 1, 2, (-1.0, 0.0, 0.0), True), (q[0] - 1, -d[0], 1, 2, (1.0, 0.0, 0.0), True),
             (q[2], -d[2], 0, 1, (0.0, 0.0, -1.0), True), (q[2] - 1, -d[2], 0, 1, (0.0, 0.0, 1.0), True)]
    for sub, (num, den, iu, iv, n, residue) in enumerate(faces):
        t = _plane_t(num, den, C, residue)
        if t is not None and _in_square(q[iu] + t * d[iu], q[iv] + t * d[iv], t, C, residue):
            out.append((t, sub, n))
    return out


def quadratic(a, b, c, C):
    """Math.fs:4-10: the far root first (for a > 0)."""
    disc = b * b - 4 * a * c
    if C.lt(disc, 0):
        return []
    if a == 0:
        raise Irrational
    sq = fsqrt(disc)
    return [(-b + sq) / (2 * a), (-b - sq) / (2 * a)]


def _facing(n, d, C):
    """`if n .* r.d < 0.0 then n else -n` (Cylinder.fs:17, Cone.fs:25); an exact 0 is not decidable in doubles after normalise."""
    dot = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
    u = _unit(n)
    return u if C.lt(dot, 0, eq_ok=False) else (-u[0], -u[1], -u[2])


def sphere(o, d, C):
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    b = 2 * (o[0] * d[0] + o[1] * d[1] + o[2] * d[2])
    c = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - 1
    return [(t, k, _unit((o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]))) for k, t in enumerate(quadratic(a, b, c, C))]


def cylinder(o, d, C, first_sub=0):
    a = d[0] * d[0] + d[2] * d[2]
    b = 2 * (o[0] * d[0] + o[2] * d[2])
    c = o[0] * o[0] + o[2] * o[2] - 1
    out = []
    for k, t in enumerate(quadratic(a, b, c, C)):
        py = o[1] + t * d[1]
        if C.ge(py, 0, deps=(t,)) and C.le(py, 1, deps=(t,)):
            out.append((t, first_sub + k, _facing((o[0] + t * d[0], 0, o[2] + t * d[2]), d, C)))
    return out


def cone(o, d, C):
    oy = o[1] - 1
    a = d[0] * d[0] + d[2] * d[2] - d[1] * d[1]
    b = 2 * (o[0] * d[0] + o[2] * d[2] - oy * d[1])
    c = o[0] * o[0] + o[2] * o[2] - oy * oy
    out = []
    for k, t in enumerate(quadratic(a, b, c, C)):
        px, py, pz = o[0] + t * d[0], oy + t * d[1], o[2] + t * d[2]
        if C.ge(py + 1, 0, deps=(t,)) and C.le(py + 1, 1, deps=(t,)):
            apex = px == 0 and py == 0 and pz == 0                # normalise leaves the zero vector alone, whatever the facing test says
            out.append((t, k, (0.0, 0.0, 0.0) if apex else _facing((px, -py, pz), d, C)))
    return out


def solid_cylinder(o, d, C):
    """Cylinder.fs:25-29: top (the circle translated to y = 1), bottom (the circle rotated 180 degrees about z: an exact circle
    facing down here), sides."""
    out = []
    t = _plane_t(-(o[1] - 1), d[1], C)
    if t is not None and _in_circle(o[0] + t * d[0], o[2] + t * d[2], t, C):
        out.append((t, 0, (0.0, 1.0, 0.0)))
    t = _plane_t(o[1], -d[1], C, residue=True)
    if t is not None and _in_circle(o[0] + t * d[0], o[2] + t * d[2], t, C, residue=True):
        out.append((t, 1, (0.0, -1.0, 0.0)))
    return out + cylinder(o, d, C, first_sub=2)


PRIMITIVES = {"plane": plane, "square": square, "circle": circle, "cube": cube, "sphere": sphere, "cylinder": cylinder, "cone": cone,
              "solidCylinder": solid_cylinder}
RESIDUE_FACES = {("cube", 2), ("cube", 3), ("cube", 4), ("cube", 5), ("solidCylinder", 1)}
FLAT = {("plane", 0), ("square", 0), ("circle", 0), ("solidCylinder", 0), ("solidCylinder", 1)} | {("cube", k) for k in range(6)}


def axis_map(ops):
    """x_world = s * x_model + tr per axis, for a list of translations and per-axis scales (first listed applied first)."""
    s, tr = [F(1)] * 3, [F(0)] * 3
    for op in ops:
        v = op[1] if isinstance(op[1], (tuple, list)) else (op[1],) * 3
        v = [F(c) for c in v]
        if op[0] == "scale":
            s, tr = [a * b for a, b in zip(s, v)], [a * b for a, b in zip(tr, v)]
        else:
            assert op[0] == "translate", "the exact families hold no rotations"
            tr = [a + b for a, b in zip(tr, v)]
    return s, tr


def leaf_hits(prim, o, d, C):
    """The hits of ("prim", kind, ops, i) for the world ray (o, d): Transform.fs:80-87 around the model-frame primitive."""
    _, kind, ops, i = prim
    s, tr = axis_map(ops)
    om = tuple((a - b) / c for a, b, c in zip(o, tr, s))
    dm = tuple(a / c for a, c in zip(d, s))
    out = []
    name = KIND_NAME[kind]
    for t, sub, n in PRIMITIVES[name](om, dm, C):
        nw = _unit([n[k] / float(s[k]) for k in range(3)])        # the inverse transpose of a per-axis scale, then normalise
        out.append(Hit(t, i, sub, False, np.array(nw), (name, sub) in RESIDUE_FACES, (kind, tuple(ops), sub)))
    return out


# ---- Csg.fs:19-94 ------------------------------------------------------------------------------------------------------------------

TAKE, DISCARD, FLIP = "Take", "Discard", "Flip"
RULES = {
    ft.UNION: {"OutsideIntoA": TAKE, "OutsideIntoB": TAKE, "AIntoOutside": TAKE, "BIntoOutside": TAKE},
    ft.SUBTRACT: {"OutsideIntoA": TAKE, "AIntoAB": FLIP, "ABleaveB": FLIP, "AIntoOutside": TAKE},
    ft.INTERSECT: {"BIntoAB": TAKE, "AIntoAB": TAKE, "ABleaveA": TAKE, "ABleaveB": TAKE},
    ft.EXCLUDE: {"OutsideIntoA": TAKE, "OutsideIntoB": TAKE, "BIntoAB": FLIP, "AIntoAB": FLIP, "ABleaveA": FLIP, "ABleaveB": FLIP,
                 "AIntoOutside": TAKE, "BIntoOutside": TAKE},
}
INTERSECTION_TYPE = {("A", True, True): "ABleaveA", ("A", False, True): "BIntoAB", ("A", True, False): "AIntoOutside", ("A", False, False): "OutsideIntoA",
                     ("B", True, True): "ABleaveB", ("B", False, True): "BIntoOutside", ("B", True, False): "AIntoAB", ("B", False, False): "OutsideIntoB"}


def _rec_pair(C, g, h):
    """t against t.  Two hits with one key come from primitives built by the same calls, through the same sub-face: the same arithmetic
    on the same inputs, the same bits whatever t is (Family I rests on this) - their equality needs no exact t."""
    if g.key is not None and g.key == h.key and g.t == h.t:
        return
    C.rec(g.t, h.t, residue=g.res or h.res)


def _flip(h):
    return h._replace(flip=not h.flip, n=-np.asarray(h.n))


def constructed_solid(op, a_hits, b_hits, C=None, types=None):
    """Csg.fs:74-94.  `types`, when given, collects the intersection type of every merged hit."""
    tagged = [(h, "A") for h in a_hits] + [(h, "B") for h in b_hits]
    if C is not None:                                              # whatever pairs the sort compares are among these
        for i in range(len(tagged)):
            for j in range(i + 1, len(tagged)):
                _rec_pair(C, tagged[i][0], tagged[j][0])
    merged = sorted(tagged, key=lambda v: v[0].t)                  # stable, as Seq.sortBy is
    rules = RULES[op]
    out, in_a, in_b = [], False, False
    for h, side in merged:
        ty = INTERSECTION_TYPE[(side, in_a, in_b)]
        action = rules.get(ty, DISCARD)
        if types is not None:
            types.append(ty)
        if side == "A":
            in_a = not in_a
        else:
            in_b = not in_b
        if action == TAKE:
            out.append(h)
        elif action == FLIP:
            out.append(_flip(h))
    return out


def closest(hits, C=None):
    """Scene.fs:112-116: stable sort, skip while 0 > t, the head."""
    if C is not None:
        for i, h in enumerate(hits):
            C.rec(h.t, 0, residue=h.res)
            for g in hits[i + 1:]:
                _rec_pair(C, h, g)
    for h in sorted(hits, key=lambda h: h.t):
        if not 0 > h.t:
            return h
    return None


def light_is_blocked(hits, max_dist, C=None):
    """Scene.fs:119-121 (every material of these scenes applies lighting)."""
    if C is not None:
        for h in hits:
            C.rec(h.t, 0, residue=h.res)
            C.rec(h.t, max_dist, residue=h.res)
    return any(h.t >= 0 and h.t < max_dist for h in hits)


def evaluate(tree, leaf):
    """The hit sequence of a tree (Scene.fs:67-104); leaf(prim) gives a primitive's hits, C its comparisons' list (or None)."""
    def walk(t):
        if t[0] == "prim":
            return leaf(t)
        if t[0] == "group":
            return [h for c in t[1] for h in walk(c)]
        assert t[0] == "csg"
        return constructed_solid(t[1], walk(t[2]), walk(t[3]), leaf.C)
    return walk(tree)


# ---- Family II: lattice rays through lattice targets ---------------------------------------------------------------------------------

DIR_SET = [F(1, 4), F(1, 2), F(1), F(2)]
BARE = ()
XF = (("scale", (2, F(1, 2), 4)), ("translate", (F(1, 4), F(-3, 2), 3)))
MIRROR = (("scale", (-1, 2, F(-1, 2))), ("translate", (F(-1, 2), F(1, 8), 1)))
TRANSFORMS = {"bare": BARE, "scaled": XF, "mirrored": MIRROR}


def eighths(lo, hi, open_ends=False):
    v = [F(k, 8) for k in range(int(F(lo) * 8), int(F(hi) * 8) + 1)]
    return [x for x in v if not open_ends or (x != lo and x != hi)]


AXIS4 = [(1, 0), (-1, 0), (0, 1), (0, -1)]
H2 = F(1, 2)


def _cube_points(which):
    pts = []
    for x in eighths(-H2, H2):
        for y in eighths(-H2, H2):
            for z in eighths(-H2, H2):
                n_face = sum(abs(c) == H2 for c in (x, y, z))
                if n_face == which:
                    pts.append((x, y, z))
    return pts


def single_classes(kind):
    """name -> (target points in the model frame, what the target hit must be: "hit", "miss", "double", "tangent", None)."""
    e01, inner = eighths(0, 1), eighths(0, 1, True)
    disc = [(x, z) for x in eighths(-1, 1) for z in eighths(-1, 1) if x * x + z * z < 1]
    if kind == "plane":
        return {"any": ([(x, 0, z) for x in eighths(-1, 1) for z in eighths(-1, 1)], "hit")}
    if kind == "square":
        return {"border": ([(u, 0, v) for u in e01 for v in e01 if u in (0, 1) or v in (0, 1)], "hit"),
                "inside": ([(u, 0, v) for u in inner for v in inner], "hit")}
    if kind == "circle":
        return {"rim": ([(x, 0, z) for x, z in AXIS4], "miss"), "inside": ([(x, 0, z) for x, z in disc], "hit")}
    if kind == "cylinder":
        return {"rim": ([(x, y, z) for x, z in AXIS4 for y in (0, 1)], "hit"), "side": ([(x, y, z) for x, z in AXIS4 for y in inner], "hit")}
    if kind == "solidCylinder":
        return {"rim_top": ([(x, 1, z) for x, z in AXIS4], "hit"), "rim_bottom": ([(x, 0, z) for x, z in AXIS4], "hit"),
                "caps": ([(x, y, z) for x, z in disc for y in (0, 1)], "hit"), "side": ([(x, y, z) for x, z in AXIS4 for y in inner], "hit")}
    if kind == "cone":
        return {"rim": ([(x, 0, z) for x, z in AXIS4], "hit"), "apex": ([(0, 1, 0)], "double"),
                "side": ([(x * (1 - y), y, z * (1 - y)) for x, z in AXIS4 for y in inner], "hit")}
    if kind == "sphere":
        axis = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
        return {"axis": (axis, "hit"), "tangent": (axis, "tangent")}
    assert kind == "cube"
    return {"face": (_cube_points(1), "hit"), "edge": (_cube_points(2), "hit"), "corner": (_cube_points(3), "hit")}


def pair_case(name):
    """name -> (A, B, classes) with A and B as (kind, own ops): solids that touch or share faces."""
    inner = eighths(-H2, H2, True)
    if name == "cubes":                                            # a shared face at x = 1/2
        return ("cube", ()), ("cube", (("translate", (1, 0, 0)),)), {
            "shared_face": ([(H2, y, z) for y in inner for z in inner], "hit"),
            "shared_edge": ([(H2, y, z) for y in eighths(-H2, H2) for z in eighths(-H2, H2) if abs(y) == H2 or abs(z) == H2], "hit")}
    if name == "walls":                                            # B inside A, its four side walls in A's
        low = eighths(-F(1, 4), F(1, 4), True)
        return ("cube", ()), ("cube", (("scale", (1, H2, 1)),)), {
            "wall": ([(sx * H2, y, z) for sx in (1, -1) for y in low for z in inner] + [(x, y, sz * H2) for sz in (1, -1) for y in low for x in inner], "hit"),
            "lid": ([(x, sy * F(1, 4), z) for sy in (1, -1) for x in inner for z in inner], "hit")}
    if name == "spheres":                                          # touching at (1, 0, 0)
        return ("sphere", ()), ("sphere", (("translate", (2, 0, 0)),)), {
            "touch": ([(1, 0, 0)], "hit"), "touch_near": ([(1, 0, 0)], "hit", {"kmax": 1, "dirs": DIR_SET[:2], "n": 320}), "poles": ([(-1, 0, 0), (3, 0, 0), (0, 1, 0), (2, -1, 0), (0, 0, 1), (2, 0, -1)], "hit")}
    if name == "cylinders":                                        # B on top of A: the rim at y = 1 is both A's upper and B's lower
        return ("cylinder", ()), ("cylinder", (("translate", (0, 1, 0)),)), {
            "shared_rim": ([(x, 1, z) for x, z in AXIS4], "hit"),
            "side": ([(x, y, z) for x, z in AXIS4 for y in eighths(0, 2, True) if y != 1], "hit")}
    if name == "cones":                                            # identical cones: through the apex all four roots are one t (A0 = A1 = B0 = B1)
        inner01 = eighths(0, 1, True)
        return ("cone", ()), ("cone", ()), {
            "apex": ([(0, 1, 0)], "double"), "rim": ([(x, 0, z) for x, z in AXIS4], "hit"),
            "side": ([(x * (1 - y), y, z * (1 - y)) for x, z in AXIS4 for y in inner01], "hit")}
    if name == "tangent":                                          # identical spheres: a tangent ray has A0 = A1 = B0 = B1
        axis = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
        return ("sphere", ()), ("sphere", ()), {"tangent": (axis, "tangent"), "axis": (axis, "hit")}
    assert name == "capped"                                        # the solidCylinder's top cap and a circle in the same place
    disc = [(x, z) for x in eighths(-1, 1) for z in eighths(-1, 1) if x * x + z * z < 1]
    return ("solidCylinder", ()), ("circle", (("translate", (0, 1, 0)),)), {
        "cap": ([(x, 1, z) for x, z in disc], "hit"), "rim": ([(x, 1, z) for x, z in AXIS4], "hit")}


PAIRS = ["cubes", "walls", "spheres", "cylinders", "capped", "cones", "tangent"]
SINGLES = ["plane", "square", "circle", "cylinder", "solidCylinder", "cone", "sphere", "cube"]


def to_world(p, ops):
    s, tr = axis_map(ops)
    return tuple(F(c) * a + b for c, a, b in zip(p, s, tr))


def lattice_rays(points, ops, n, seed, tangent=False, kmax=8, dirs=None):
    """n rays o = P - k d through world targets P (model points under `ops`): d from +-{1/4, 1/2, 1, 2} per component, k in 0 .. 8;
    one ray in eight runs away from its target (k = -1 .. -8: every t of the target is negative).  tangent: d perpendicular to the
    model-frame radius of the sphere's axis point P (the one class with a zero component; its scenes hold no plane).  kmax, dirs: a
    class of short rays (the touching spheres: most of them start inside A, so that the touching point is the closest hit)."""
    rng = np.random.default_rng(seed)
    dirs = DIR_SET if dirs is None else dirs
    s, _ = axis_map(ops)
    rays = []
    for _ in range(n):
        pm = points[int(rng.integers(len(points)))]
        P = to_world(pm, ops)
        d = [dirs[int(rng.integers(len(dirs)))] * int(rng.choice([-1, 1])) for _ in range(3)]
        if tangent:
            axis = [k for k in range(3) if pm[k] != 0][0]
            d[axis] = F(0)
        k = int(rng.integers(0, kmax + 1))
        if rng.integers(8) == 0:
            k = -int(rng.integers(1, kmax + 1))
        rays.append((tuple(P[a] - k * d[a] for a in range(3)), tuple(d), k))
    return rays


def rays_as_arrays(rays):
    o = np.array([[float(c) for c in r[0]] for r in rays])
    d = np.array([[float(c) for c in r[1]] for r in rays])
    assert all(F(x) == c for r, row in zip(rays, o) for x, c in zip(row, r[0]))
    return o, d, np.array([r[2] for r in rays])


class LeafCache:
    """The exact hits of every primitive for a fixed list of rays, computed once and shared by all operators and shapes."""

    def __init__(self, rays):
        self.rays, self.store = rays, {}

    def leaf_fn(self, index, C):
        def leaf(prim):
            key = (prim[1], tuple(prim[2]), index)
            if key not in self.store:
                c = Cmps()
                try:
                    hits = leaf_hits((prim[0], prim[1], prim[2], -1), self.rays[index][0], self.rays[index][1], c)
                except Irrational:
                    hits = None
                self.store[key] = (hits, c)
            hits, c = self.store[key]
            if hits is None:
                raise Irrational
            C.extend(c)
            leaf.seen.extend(h.t for h in hits)
            return [h._replace(leaf=prim[3]) for h in hits]
        leaf.C, leaf.seen = C, []
        return leaf


Verdict = namedtuple("Verdict", "kept residue hits winner tied")


def judge(tree, cache, index):
    """One ray against one scene tree: whether the ray is kept, whether it is a residue ray, its exact hit sequence, the winner of
    `closest`, and whether the winner's t is shared by another hit of some primitive (a hit that CSG threw away counts: the tie was
    decided inside the node)."""
    C = Cmps()
    leaf = cache.leaf_fn(index, C)
    try:
        hits = evaluate(tree, leaf)
    except Irrational:
        return Verdict(False, False, None, None, False)
    w = closest(hits, C)
    tied = w is not None and sum(t == w.t for t in leaf.seen) > 1
    return Verdict(robust(C), has_residue_equality(C), hits, w, tied)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------

FILLER_AT = [(41, F(3, 8), -37), (-39, F(-163, 4), F(5, 8))]       # about 40 units out, off every lattice line through a target
FAR_AT = (37, F(-165, 4), 300)
FILLERS = [("prim", ft.SPHERE, (("scale", (F(1, 4),) * 3), ("translate", FILLER_AT[k])), 20 + k) for k in range(2)]
FAR = ("prim", ft.SPHERE, (("scale", (F(1, 4),) * 3), ("translate", FAR_AT)), 22)
SHAPES = ["fold", "list_a", "list_b", "merge", "nested"]


def prim(kind, ops, i):
    return ("prim", H.PRIMS[kind] if isinstance(kind, str) else kind, tuple(ops), i)


def shaped(shape, op, A, B, op2=None):
    """The target item for operands A and B (leaves 0 and 1): "fold" a pair on its own (OP_CSG_PAIR straight into the query), "list_a" /
    "list_b" the pair as operand A / B of a union with a far-away sphere (union passes an operand through when the other has no hit: the
    pair's list mode), "merge" each operand in a one-child group (not bare: csg_merge), "nested" op(op2(A, B), B') with B' a copy of B
    as leaf 2 (ties across both levels)."""
    pair = ("csg", op, A, B)
    if shape == "fold":
        return pair
    if shape == "list_a":
        return ("csg", ft.UNION, pair, FAR)
    if shape == "list_b":
        return ("csg", ft.UNION, FAR, pair)
    if shape == "merge":
        return ("csg", op, ("group", [A]), ("group", [B]))
    assert shape == "nested"
    return ("csg", op, ("csg", op2, A, B), ("prim", B[1], B[2], 2))


def scene_tree(target):
    return ("group", [target] + FILLERS)


def float_ops(ops):
    return [(k, tuple(float(c) for c in v) if isinstance(v, (tuple, list)) else float(v), *rest) for k, v, *rest in ops]


def float_tree(tree):
    if tree[0] == "prim":
        return ("prim", tree[1], float_ops(tree[2]), tree[3])
    if tree[0] == "group":
        return ("group", [float_tree(t) for t in tree[1]])
    return ("csg", tree[1], float_tree(tree[2]), float_tree(tree[3]))


def build_scene(b, target, lights=True):
    """The target and the two fillers as three top-level items (three items: bundle_cull and exact_cull are in play)."""
    b.clear()
    b.set_objects(b.group([build_tree(b, float_tree(t)) for t in [target] + FILLERS]))
    if lights:
        b.add_directional((0.3, -1.0, 0.5), (1, 1, 1))
        b.add_positional((1.0, 6.0, -2.0), (1.0, 0.01, 0.02), (0.6, 0.6, 0.6))
    b.commit()


def expected_facts(shape):
    """What limit_tools.tree_facts must say of a shape's target: (marks live at most, marks under its fused pair; -1: no pair)."""
    return {"fold": (0, 0), "list_a": (2, 1), "list_b": (2, 2), "merge": (2, -1), "nested": (2, 1)}[shape]


# ---- Family I: identical operands under any transform ---------------------------------------------------------------------------------

SHEAR = (("scale", (1.3, 0.7, 1.1)), ("rotate", (1.0, 2.0, 0.5), 0.8), ("scale", (0.9, 1.4, 0.6)), ("translate", (0.2, 0.1, -0.3)))


def identical_operands(kind):
    """X and X' by the same calls; the plane only as operand B of the square under the same transforms (the square's hit is the plane's,
    filtered: the same bits)."""
    if kind == "plane":
        return prim("square", SHEAR, 0), prim("plane", SHEAR, 1)
    return prim(kind, SHEAR, 0), prim(kind, SHEAR, 1)


def family1_rays(kind, n=1536, seed=5):
    """helpers.random_rays toward the operand; no direction component is zero (checked)."""
    o, d = H.random_rays(n, seed=seed + len(kind), origin_scale=3.0, toward=(0.3, 0.3, -0.1), spread=0.5 if kind in ("square", "plane", "circle") else 0.8)
    assert np.all(d != 0.0)
    return o, d


class OracleLeaves:
    """Family I's leaf provider: a primitive's own hit sequence as the oracle gives it for the scene that holds nothing else."""

    C = None

    def __init__(self, orc, o, d, index=None):
        self.orc, self.o, self.d, self.store, self.index = orc, o, d, {}, index

    def at(self, index):
        other = OracleLeaves(self.orc, self.o, self.d, index)
        other.store = self.store
        return other

    def __call__(self, p):
        key = (p[1], tuple(p[2]))
        if key not in self.store:
            b = self.orc
            b.clear()
            b.set_objects(b.group([build_tree(b, ("prim", p[1], list(p[2]), 0))]))
            b.commit()
            self.store[key] = b.all_hits(self.o, self.d, cap=8)
        counts, t, _, n = self.store[key]
        i = self.index
        return [Hit(float(t[i, k]), p[3], None, False, n[i, k].copy(), False, None) for k in range(counts[i])]

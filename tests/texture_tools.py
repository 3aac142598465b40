"""An independent reference for texture lookups, and the cases of tests/test_texture_edges.py.

The reference restates, over Python floats (binary64, no contraction), Textures/Texture.fs:8-29 (repeat, the uv functions, grid),
Textures/Image.fs:27-35 (nearest texel, with the one stated deviation: an index past the last byte reads the last texel, a NaN
coordinate texel 0), Sphere.fs:6-10 and Plane.fs:28-33, in the primitive's model frame.  It shares nothing with oracle/ or the
device.  Cube side faces and the solidCylinder's bottom cap follow the convention of tests/tie_tools.py: the residue-free geometry
(DESIGN.md §3), i.e. a cube face is the unit square in (x, z), (y, z) or (x, y) of the cube's [0, 1]^3 frame and the bottom cap has
u = -x.

A restatement in floats is exact wherever no step of the device can be fused or reordered into another rounding.  On the exact
families that is proved per case with fractions.Fraction (`prove_face_case`, `prove_dyadic`): every value on the way to (u, v) is a
double, so every sum and product up to there is exact, fused or not, and from (u, v) on each step is a single correctly rounded
operation (a division by the uv scale, `x - floor x`, `ru * width`) or an exact one (floor, abs, sums of small integers).

Where (u, v) goes through libm or a rotation nothing is exact: there the coordinate is computed with mpmath at 60 digits from the
ray's exact inputs, and a point closer to a border than MARGIN * max(1, |coordinate|) is undecided (the ladders)."""
import itertools
import math
from collections import namedtuple
from fractions import Fraction as F

import mpmath
import numpy as np

import functracer_amd as ft

from . import helpers as H
from .tie_tools import is_small_dyadic

mpmath.mp.dps = 60
MARGIN = 2.0 ** -46               # 64 ulp of 1.0: a libm error of a few ulp plus the formula's three roundings, with headroom; not tuned
MAX_UNDECIDED = 0.25
LIGHT = ((0.0, -1.0, 0.0), (1.0, 1.0, 1.0))   # the one light: an unlit material's colour comes back from getColourForRay once, times nothing


# ---- the reference --------------------------------------------------------------------------------------------------------------------

def ffloor(x):
    """floor as IEEE has it (math.floor raises on inf and NaN and returns an int)."""
    if x != x or math.isinf(x) or abs(x) >= 2.0 ** 52:
        return x
    return float(math.floor(x))


def fdiv(x, y):
    """x / y as IEEE has it (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(x) / np.float64(y))


def fsub(x, y):
    with np.errstate(all="ignore"):
        return float(np.float64(x) - np.float64(y))


def repeat_one(x):                                                 # Texture.fs:9-11
    a = abs(fsub(x, ffloor(x)))
    return 1.0 - a if a < 0.0 else a


def apply_ops(ops, u, v):
    """The uv functions, outermost first (Texture.fs:14-22).  Rotations belong to the ladders and go through mpmath (`mp_rotate_uv`)."""
    for kind, a, b in ops:
        assert kind == 0.0, "the float reference holds no rotation"
        u, v = fdiv(u, a), fdiv(v, b)
    return u, v


def grid_first(u, v):
    """Texture.fs:24-29: True for colour1."""
    u, v = repeat_one(u), repeat_one(v)
    if u < 0.5 and v < 0.5:
        return True
    if u < 0.5:
        return False
    if u > 0.5 and v > 0.5:
        return True
    return False


def image_texel(w, h, u, v):
    """Image.fs:28-31: the texel (index / 3) read for (u, v); past the last byte the last texel, texel 0 for NaN."""
    u, v = repeat_one(u), repeat_one(v)
    x, y = ffloor(u * float(w)), ffloor(v * float(h))
    if x != x or y != y:
        return 0
    index = int(y) * (3 * w) + 3 * int(x)
    return min(index, 3 * (w * h - 1)) // 3


def hue(c, times=1):                                               # CommonTypes.fs:90: (r, g, b) -> (b, r, g)
    c = tuple(c)
    for _ in range(times % 3):
        c = (c[2], c[0], c[1])
    return c


def sphere_uv(n):                                                  # Sphere.fs:6-10
    return 0.5 + math.atan2(n[2], n[0]) / (2.0 * math.pi), 0.5 - math.asin(n[1]) / math.pi


class Grid(namedtuple("Grid", "c1 c2")):
    def colour(self, u, v):
        return self.c1 if grid_first(u, v) else self.c2

    def wrap(self, b, ops, child):
        return b.texture_grid(self.c1, self.c2, list(ops), child)


class Image:
    def __init__(self, w, h, seed):
        self.w, self.h = w, h
        self.px = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)

    def texel(self, k):
        return tuple(float(c) / 255.0 for c in self.px.reshape(-1, 3)[k])

    def colour(self, u, v):
        return self.texel(image_texel(self.w, self.h, u, v))

    def wrap(self, b, ops, child):
        return b.texture_image(self.px, list(ops), child)


GRID = Grid((0.9, 0.2, 0.1), (0.1, 0.3, 0.8))
IMAGE_SIZES = [(4, 2), (8, 4), (5, 7), (7, 3), (1, 1), (1, 9), (9, 1)]   # (width, height)


def image(w, h, salt=0):
    return Image(w, h, 1000 * w + 10 * h + salt)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------

def is_double(x):
    """x (a Fraction) is a finite binary64 value."""
    try:
        return F(float(x)) == x
    except OverflowError:
        return False


def prove_dyadic(*values):
    """Every value is a small dyadic: sums and products of a few of them are exact, fused or not (tie_tools.is_small_dyadic)."""
    return all(is_small_dyadic(F(v)) for v in values)


E53, E54, E60 = 2.0 ** -53, 2.0 ** -54, 2.0 ** -60
# 2^52 + 0.5 is no double (it rounds to 2^52); the representable value of that kind, an ru of exactly 0.5 far from the origin, is 2^51 + 0.5
TARGETS = [0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0, 3.5, -3.5, 0.5 + E53, 0.5 - E54, 1.0 - E53, E60, -E60,
           2.0 ** 51 + 0.5, float(2 ** 52), 1e300]
ZERO_OPS = [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, -0.0, 0.5)]

# face -> (primitive, ray axis, side the ray starts on, domain)
FACES = {"plane": ("plane", 1, 1, "any"), "square": ("square", 1, 1, "unit"), "circle": ("circle", 1, 1, "disc"),
         "cube_bottom": ("cube", 1, -1, "unit"), "cube_top": ("cube", 1, 1, "unit"), "cube_left": ("cube", 0, -1, "unit"),
         "cube_right": ("cube", 0, 1, "unit"), "cube_front": ("cube", 2, -1, "unit"), "cube_back": ("cube", 2, 1, "unit"),
         "cap_top": ("solidCylinder", 1, 1, "disc"), "cap_bottom": ("solidCylinder", 1, -1, "disc")}
LAYER_STEP = 4                                                     # copies of a primitive are stacked along the ray axis, 4 apart
XF = (("scale", (2.0, 0.5, 4.0)), ("translate", (0.25, -1.5, 3.0)))   # tie_tools.XF: powers of two and a dyadic translation


def face_ray(face, a, b):
    """The model ray (o, d) that meets `face` at t = 1 where its residue-free (u, v) is (a, b).  Along a model axis,
    so p = o + 1 * d moves one coordinate only.  Returns Fractions."""
    prim, axis, side, _ = FACES[face]
    a, b = F(a), F(b)
    h = F(1, 2)
    if prim in ("plane", "square", "circle"):
        o = [a, F(1), b]
    elif face == "cap_top":
        o = [a, F(2), b]
    elif face == "cap_bottom":
        o = [-a, F(-1), b]                                          # the circle rotated 180 degrees about z: u = -x
    else:
        start = F(3, 2) * side
        o = {1: [a - h, start, b - h], 0: [start, a - h, b - h], 2: [a - h, b - h, start]}[axis]   # (x, z), (y, z), (x, y) of the [0, 1]^3 frame
    d = [F(0)] * 3
    d[axis] = F(-side)
    return o, d


def prove_face_case(face, a, b, offset=0, xf=False):
    """Every value from the world ray to (tu, tv) is a double, so that no rounding happens whatever is fused: the origin's components;
    for the cube o + 1/2 (the device shifts to the [0, 1]^3 frame first) giving (a, b) back; along the ray axis small dyadics only
    (there t = 1 is computed: a quotient of small dyadics).  Across the axis a copy's offset adds 0 to 1 * x.  Under XF everything must
    be a small dyadic (tie_tools' Family II argument)."""
    prim, axis, side, domain = FACES[face]
    o, d = face_ray(face, a, b)
    if not all(is_double(c) for c in o) or not prove_dyadic(o[axis], offset):
        return False
    if prim == "cube" and not all(is_double(c + F(1, 2)) for k, c in enumerate(o) if k != axis):
        return False
    if xf and not prove_dyadic(*o):
        return False
    a, b = F(a), F(b)
    if domain == "unit":
        return 0 <= a <= 1 and 0 <= b <= 1
    if domain == "disc":
        return a * a + b * b <= F(31, 32)                           # inside the rim by a margin no rounding of x^2 + z^2 can cross
    return True


def world_ray(face, a, b, offset=0, xf=False):
    """The world ray as floats: the model ray moved `offset` along its axis, then under XF."""
    _, axis, _, _ = FACES[face]
    o, d = face_ray(face, a, b)
    o[axis] += offset
    if xf:
        (_, s), (_, tr) = XF
        o = [c * F(k) + F(t) for c, k, t in zip(o, s, tr)]
        d = [c * F(k) for c, k in zip(d, s)]
        assert prove_dyadic(*o, *d)
    return [float(c) for c in o], [float(c) for c in d]


def realise(x, domain, cube, small=False):
    """(p, a): a face coordinate p inside the domain and a uv scale a with fl(p / a) == x, sign of zero included.  p is x itself where
    it lies in the domain and survives the way there (a = 1); else a small dyadic p and a power of two where one exists, else the
    double nearest p / x whose single correctly rounded division gives x.  small: p must be a small dyadic (under XF)."""
    def inside(p):
        if not is_double(F(p)) or (cube and not is_double(F(p) - F(1, 2))) or (small and not prove_dyadic(p)):
            return False
        return True if domain == "any" else 0.0 <= p <= 1.0 if domain == "unit" else abs(p) <= 0.6875
    if x == 0.0:
        return (0.0, 1.0) if math.copysign(1.0, x) > 0 else (0.0, -1.0)
    if inside(x):
        return x, 1.0
    if inside(-x):
        return -x, -1.0
    for p in (0.5, 0.25, 0.375, 0.625, 0.125):
        a0 = fdiv(p, x)
        cands, lo, hi = [a0], a0, a0
        for _ in range(4):
            lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
            cands += [lo, hi]
        _, e = math.frexp(a0)
        cands = [math.ldexp(math.copysign(0.5, a0), e), math.ldexp(math.copysign(0.5, a0), e + 1)] + cands   # powers of two first
        for a in cands:
            if a != 0.0 and fdiv(p, a) == x:
                return p, a
    raise AssertionError(f"no uv scale realises {x!r}")


FaceCase = namedtuple("FaceCase", "a b ops layer target")


def face_cases(face, xf=False):
    """Every pair of TARGETS as the final (u, v) on `face`: cases grouped into layers, one per distinct uv scale.  Under XF only the
    cases whose whole ray is made of small dyadics remain.  Returns (layers: list of ops, cases)."""
    prim, _, _, domain = FACES[face]
    real = {i: realise(x, domain, prim == "cube", small=xf) for i, x in enumerate(TARGETS)}
    layers, cases = [], []
    for i, j in itertools.product(range(len(TARGETS)), repeat=2):
        (pa, sa), (pb, sb) = real[i], real[j]
        ops = () if (sa, sb) == (1.0, 1.0) else ((0.0, sa, sb),)
        if ops not in layers:
            layers.append(ops)
        cases.append(FaceCase(pa, pb, ops, layers.index(ops), (TARGETS[i], TARGETS[j])))
    return layers, cases


def zero_scale_cases(face):
    """A uv scale of 0: u / 0 is inf or NaN, NaN after repeat.  Layers are ZERO_OPS; face points are small dyadics of the domain."""
    pts = [(0.0, 0.0), (0.5, 0.25), (0.25, 0.5), (0.625, 0.0)]
    return [FaceCase(a, b, (op,), k, None) for k, op in enumerate(ZERO_OPS) for a, b in pts]


def same_bits(x, y):
    return (x == y and math.copysign(1.0, x) == math.copysign(1.0, y)) or (x != x and y != y)


def build_layers(b, face, layers, texture, xf=False, chunk=None):
    """One copy of the face's primitive per layer, `LAYER_STEP` apart along the ray axis, each under the texture with the layer's uv
    functions and ignoreLight; one directional light.  chunk = (first, count) builds a part of the layers only."""
    prim, axis, _, _ = FACES[face]
    first, count = chunk or (0, len(layers))
    b.clear()
    objs = []
    for k in range(first, min(first + count, len(layers))):
        ops = []
        if k:
            v = [0.0] * 3
            v[axis] = float(LAYER_STEP * k)
            ops.append(("translate", tuple(v)))
        if xf:
            ops += list(XF)
        node = b.primitive(H.PRIMS[prim])
        if ops:
            node = b.transform(ops, node)
        objs.append(b.ignore_light(texture.wrap(b, layers[k], node)))
    b.set_objects(b.group(objs))
    b.add_directional(*LIGHT)
    b.commit()


def layer_rays(face, cases, xf=False):
    o, d = zip(*(world_ray(face, c.a, c.b, LAYER_STEP * c.layer, xf) for c in cases))
    return np.array(o), np.array(d)


def expected_colours(cases, texture):
    return np.array([texture.colour(*apply_ops(c.ops, c.a, c.b)) for c in cases])


# ---- the image family: every texel border of every size, on the bare plane ------------------------------------------------------------

def image_cases(w, h):
    """(u, v) on the plane: k / w and k / h for every k with the doubles next to them on both sides, against generic coordinates of
    every column and row; ru == 1.0 (u = -2^-60) in every row, the last one included, and rv == 1.0: the wrap and the clamp."""
    def around(x):
        return [math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)]
    us = [x for k in range(w + 1) for x in around(k / w)]
    vs = [x for k in range(h + 1) for x in around(k / h)]
    mid_u = [(k + 0.5) / w for k in range(w)]
    mid_v = [(k + 0.5) / h for k in range(h)]
    pts = [(u, v) for u in us for v in mid_v] + [(u, v) for u in mid_u for v in vs] + [(u, v) for u in us for v in vs]
    pts += [(-E60, v) for v in mid_v + vs] + [(u, -E60) for u in mid_u + us] + [(-E60, -E60), (-E60, 1.0 - E53), (1.0 - E53, -E60)]
    return [FaceCase(u, v, (), 0, (u, v)) for u, v in pts]


# ---- the sphere's axis points ------------------------------------------------------------------------------------------------------------

AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
AXIS_UV = {(1, 0, 0): (0.5, 0.5), (-1, 0, 0): (1.0, 0.5), (0, 0, 1): (0.75, 0.5), (0, 0, -1): (0.25, 0.5), (0, 1, 0): (0.5, 0.0), (0, -1, 0): (0.5, 1.0)}
SPHERE_XF = {"unit": (), "scaled": (("scale", (2.0, 2.0, 2.0)),), "moved": (("translate", (0.25, -1.5, 3.0)),)}


def sphere_axis_rays(xf):
    """Rays o = 3 e, d = -e in the model frame (a = 1, b = -6, c = 8: roots 4 and 2, the hit at e exactly, |e| = 1 so n = e).  Returns
    (world o, world d, model normals).  On the bare sphere two more at the seam with dz = -0.0, and oz = -0.0 as well: n.z = -0.0 and
    atan2(-0, -1) = -pi, u = 0: the same texel as u = 1."""
    s = 2.0 if xf == "scaled" else 1.0
    tr = (0.25, -1.5, 3.0) if xf == "moved" else (0.0, 0.0, 0.0)
    o, d, n = [], [], []
    for e in AXES:
        o.append([3.0 * s * c + t for c, t in zip(e, tr)])
        d.append([-s * c + 0.0 for c in e])
        n.append([float(c) for c in e])
    if xf == "unit":
        o += [[-3.0, 0.0, 0.0], [-3.0, 0.0, -0.0]]
        d += [[1.0, 0.0, -0.0], [1.0, 0.0, -0.0]]
        n += [[-1.0, 0.0, 0.0 + 2.0 * -0.0], [-1.0, 0.0, -0.0 + 2.0 * -0.0]]
    assert prove_dyadic(*(c for row in o + d for c in row))
    return np.array(o), np.array(d), n


def build_single(b, node_fn, texture, ops=(), hue_shifts=0, unlit=True, extra=None):
    """One object: node_fn(b) under the texture, `hue_shifts` hueShifts and ignoreLight; the one light."""
    b.clear()
    node = texture.wrap(b, ops, node_fn(b))
    for _ in range(hue_shifts):
        node = b.hue_shift(0.0, node)
    if unlit:
        node = b.ignore_light(node)
    b.set_objects(b.group([node] + (extra(b) if extra else [])))
    b.add_directional(*LIGHT)
    b.commit()


def prim_node(kind, xf=()):
    def fn(b):
        node = b.primitive(H.PRIMS[kind])
        return b.transform(list(xf), node) if xf else node
    return fn


# ---- primitives whose (u, v) is (0, 0) -----------------------------------------------------------------------------------------------------

OCTA = [[(1, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 1, 0), (-1, 0, 0), (0, 0, 1)], [(-1, 0, 0), (0, -1, 0), (0, 0, 1)], [(0, -1, 0), (1, 0, 0), (0, 0, 1)],
        [(0, 1, 0), (1, 0, 0), (0, 0, -1)], [(-1, 0, 0), (0, 1, 0), (0, 0, -1)], [(0, -1, 0), (-1, 0, 0), (0, 0, -1)], [(1, 0, 0), (0, -1, 0), (0, 0, -1)]]


def flat_uv_nodes():
    """name -> (node builder, rays): cone, cylinder, the solidCylinder's side (horizontal rays between its caps), a bare triangle and an
    octahedron as bspMesh 0 and bspMesh 2."""
    tris = np.array(OCTA, dtype=np.float64).reshape(-1, 9)
    o, d = H.random_rays(192, seed=7, origin_scale=3.0, toward=(0, 0.4, 0), spread=0.4)
    rng = np.random.default_rng(8)
    ang = rng.uniform(0, 2 * math.pi, 192)
    so = np.stack([3 * np.cos(ang), rng.uniform(0.05, 0.95, 192), 3 * np.sin(ang)], axis=1)
    sd = np.stack([-np.cos(ang) + rng.normal(size=192) * 0.1, np.zeros(192), -np.sin(ang) + rng.normal(size=192) * 0.1], axis=1)
    to, td = H.random_rays(192, seed=9, origin_scale=3.0, toward=(0.3, 0.3, 0.3), spread=0.2)
    return {"cone": (prim_node("cone"), (o, d)), "cylinder": (prim_node("cylinder"), (o, d)), "solidCylinder_side": (prim_node("solidCylinder"), (so, sd)),
            "triangle": (lambda b: b.triangle(*OCTA[0]), (to, td)), "bspMesh0": (lambda b: b.bsp_mesh(0, tris), (o, d)),
            "bspMesh2": (lambda b: b.bsp_mesh(2, tris), (o, d))}


FLAT_OPS = [(), ((0.0, 0.5, -2.0),), ((0.0, 0.3, 0.7), (1.0, H.deg(30.0), 0.0))]


# ---- several images in one scene ---------------------------------------------------------------------------------------------------------

def image_set():
    """Five images, in an order that puts each after the first at a byte offset that is no multiple of 4: 3, 66, 171, 198."""
    imgs = [image(1, 1, 1), image(7, 3, 2), image(5, 7, 3), image(1, 9, 4), image(9, 1, 5)]
    bases = list(itertools.accumulate([0] + [3 * i.w * i.h for i in imgs]))[:-1]
    assert bases == [0, 3, 66, 171, 198] and all(x % 4 for x in bases[1:])
    return imgs


def build_image_stack(b):
    """Squares stacked along y, 4 apart, top first: image 0 .. 4 each on its own square; then ONE node of image 2 over a group of two
    squares; a grid; and two nodes with the bytes of image 1.  Returns the texture of every square (layer k at y = -4 k)."""
    imgs = image_set()
    twin = Image(7, 3, 0)
    twin.px = imgs[1].px.copy()
    b.clear()
    sq = lambda k: b.translate((0.0, -4.0 * k, 0.0), b.primitive(ft.SQUARE)) if k else b.primitive(ft.SQUARE)
    objs = [imgs[k].wrap(b, (), sq(k)) for k in range(5)]
    objs.append(imgs[2].wrap(b, (), b.group([sq(5), sq(6)])))
    objs.append(GRID.wrap(b, (), sq(7)))
    objs += [twin.wrap(b, (), sq(8)), imgs[1].wrap(b, (), sq(9))]
    b.set_objects(b.group([b.ignore_light(n) for n in objs]))
    b.add_directional(*LIGHT)
    b.commit()
    return imgs + [imgs[2], imgs[2], GRID, twin, imgs[1]]


def image_stack_cases(textures):
    """Every texel centre of every square's image (the grid: sixteenths), as layer cases on the square."""
    cases = []
    for k, t in enumerate(textures):
        w, h = (t.w, t.h) if isinstance(t, Image) else (4, 4)
        for x in range(w):
            for y in range(h):
                u, v = (x + 0.5) / w, (y + 0.5) / h
                cases.append(FaceCase(u, v, (), -k, (u, v)))       # layer -k: the stack goes down
    return cases


# ---- function order ---------------------------------------------------------------------------------------------------------------------------

FUNCTIONS = ["material", "texture_grid", "texture_image", "hue_shift", "ignore_light"]
SEQUENCES = [s for n in range(1, 5) for s in itertools.product(FUNCTIONS, repeat=n)]
ORDER_POINT = (0.25, 0.75)                                         # grid: ru < 0.5 and rv > 0.5 -> colour2; a 2x2 image: texel 2
PER_SCENE = 60


def order_palette(pos):
    """The colours of the function at position `pos` of a sequence: material, grid c1, grid c2, the four texels of a 2x2 image."""
    base = 8 * pos
    col = lambda k: ((17 + 29 * (base + k)) % 256, (91 + 53 * (base + k)) % 256, (201 + 71 * (base + k)) % 256)
    px = np.array([col(3 + k) for k in range(4)], dtype=np.uint8).reshape(2, 2, 3)
    return tuple(c / 255.0 for c in col(0)), tuple(c / 255.0 for c in col(1)), tuple(c / 255.0 for c in col(2)), px


def order_expected(seq):
    """(material colour at ORDER_POINT, lit) by the text: every function maps the hit's material (Ray.fs:47-59), innermost first."""
    colour, lit = (1.0, 1.0, 1.0), True                               # Ray.mattWhite
    for pos, f in enumerate(seq):
        mat, c1, c2, px = order_palette(pos)
        if f == "material":
            colour, lit = mat, True
        elif f == "texture_grid":
            colour = c1 if grid_first(*ORDER_POINT) else c2
        elif f == "texture_image":
            colour = tuple(float(c) / 255.0 for c in px.reshape(-1, 3)[image_texel(2, 2, *ORDER_POINT)])
        elif f == "hue_shift":
            colour = hue(colour)
        else:
            lit = False
    return colour, lit


def build_order_scene(b, seqs):
    """Unit squares at (2 i, 0, 2 j), each wrapped by its sequence, the first function innermost.  Returns the rays, one per square."""
    b.clear()
    objs, o = [], []
    for k, seq in enumerate(seqs):
        i, j = k % 8, k // 8
        node = b.translate((2.0 * i, 0.0, 2.0 * j), b.primitive(ft.SQUARE)) if k else b.primitive(ft.SQUARE)
        for pos, f in enumerate(seq):
            mat, c1, c2, px = order_palette(pos)
            if f == "material":
                node = b.material(node, colour=mat, roughness=0.0, reflectance=0.0, shineyness=0.0)
            elif f == "texture_grid":
                node = b.texture_grid(c1, c2, [], node)
            elif f == "texture_image":
                node = b.texture_image(px, [], node)
            elif f == "hue_shift":
                node = b.hue_shift(0.0, node)
            else:
                node = b.ignore_light(node)
        objs.append(node)
        o.append([2.0 * i + ORDER_POINT[0], 1.0, 2.0 * j + ORDER_POINT[1]])
    b.set_objects(b.group(objs))
    b.add_directional((0.25, -1.0, 0.5), (1.0, 0.5, 0.25))
    b.commit()
    o = np.array(o)
    return o, np.tile([0.0, -1.0, 0.0], (len(seqs), 1))


def order_scenes():
    return [SEQUENCES[k:k + PER_SCENE] for k in range(0, len(SEQUENCES), PER_SCENE)]


# ---- ladders: borders that lie behind libm or a rotation -------------------------------------------------------------------------------------

Rung = namedtuple("Rung", "o d coord other decided side")           # side: which side of the border (+1 / -1) the exact coordinate lies on
LADDER_K = range(10, 53)


def mp_vec(v):
    return [mpmath.mpf(float(c)) for c in v]


def mp_sphere_uv(o, d):
    """(u, v) of the closest hit of the ray with the unit sphere, exactly from the doubles of (o, d)."""
    o, d = mp_vec(o), mp_vec(d)
    a = sum(c * c for c in d)
    b = 2 * sum(p * q for p, q in zip(o, d))
    c = sum(p * p for p in o) - 1
    t = (-b - mpmath.sqrt(b * b - 4 * a * c)) / (2 * a)
    p = [x + t * y for x, y in zip(o, d)]
    l = mpmath.sqrt(sum(x * x for x in p))
    n = [x / l for x in p]
    return mpmath.mpf(0.5) + mpmath.atan2(n[2], n[0]) / (2 * mpmath.pi), mpmath.mpf(0.5) - mpmath.asin(n[1]) / mpmath.pi


def _sphere_ray(u, v):
    """A ray from outside toward the sphere's point with texture coordinates (u, v) (mpmath values), its numbers rounded to doubles."""
    phi, theta = 2 * mpmath.pi * (u - mpmath.mpf(0.5)), mpmath.pi * (mpmath.mpf(0.5) - v)
    n = [mpmath.cos(theta) * mpmath.cos(phi), mpmath.sin(theta), mpmath.cos(theta) * mpmath.sin(phi)]
    nd = [float(c) for c in n]
    return [3.0 * c for c in nd], [-c for c in nd]


def decide(coord, border):
    return abs(coord - border) >= MARGIN * max(1.0, abs(float(coord)))


def sphere_ladder(which, border, other):
    """Rungs across `border` of u (which = 0) or v (1) at about +-2^-k, the other coordinate held at the generic `other`."""
    rungs = []
    for k in LADDER_K:
        for s in (1, -1):
            want = mpmath.mpf(border) + s * mpmath.mpf(2) ** -k
            o, d = _sphere_ray(want, mpmath.mpf(other)) if which == 0 else _sphere_ray(mpmath.mpf(other), want)
            uv = mp_sphere_uv(o, d)
            coord = uv[which]
            if which == 0 and border == 1.0 and coord < 0.25:        # past the seam u starts again at 0: measure from 1
                coord = coord + 1
            rungs.append(Rung(o, d, coord, uv[1 - which], decide(coord, border), 1 if coord > border else -1))
    return rungs


def mp_rotate_uv(angle, x, z):
    """Texture.rotate by the double `angle` (Texture.fs:18-22, Transform.fs:60-69 about (0, 1, 0)): exact cos and sin of that double."""
    a = mpmath.mpf(float(angle))
    c, s = mpmath.cos(a), mpmath.sin(a)
    x, z = mpmath.mpf(float(x)), mpmath.mpf(float(z))
    return c * x + s * z, -s * x + c * z


def rotated_plane_ladder(angle, border=0.5, other=0.3):
    """The plane under a rotate uv function: straight-down rays onto (x, z) whose rotated u steps across `border`, v near `other`."""
    a = mpmath.mpf(float(angle))
    c, s = mpmath.cos(a), mpmath.sin(a)
    rungs = []
    for k in LADDER_K:
        for sgn in (1, -1):
            u, v = mpmath.mpf(border) + sgn * mpmath.mpf(2) ** -k, mpmath.mpf(other)
            x, z = float(c * u - s * v), float(s * u + c * v)        # the inverse rotation, rounded
            uv = mp_rotate_uv(angle, x, z)
            rungs.append(Rung([x, 1.0, z], [0.0, -1.0, 0.0], uv[0], uv[1], decide(uv[0], border), 1 if uv[0] > border else -1))
    return rungs


CUBE_AXIS, CUBE_ANGLE = (1.0, 1.0, 0.0), H.deg(35.0)


def _mp_rotation(axis, angle):
    """Transform.fs:60-69 over mpmath, the axis normalised exactly."""
    ax = mp_vec(axis)
    l = mpmath.sqrt(sum(c * c for c in ax))
    ux, uy, uz = [c / l for c in ax]
    a = mpmath.mpf(float(angle))
    c, s = mpmath.cos(a), mpmath.sin(a)
    ic = 1 - c
    return [[c + ic * ux * ux, ic * ux * uy - s * uz, ic * ux * uz + s * uy],
            [ic * ux * uy + s * uz, c + ic * uy * uy, ic * uy * uz - s * ux],
            [ic * ux * uz - s * uy, ic * uy * uz + s * ux, c + ic * uz * uz]]


def _mp_apply(m, v):
    return [sum(m[r][k] * v[k] for k in range(3)) for r in range(3)]


def rotated_cube_ladder(border=0.5, other=0.3):
    """A cube rotated about (1, 1, 0) by 35 degrees: rays onto its top face (model y = 1/2, from above along -y in the model frame)
    whose x of the [0, 1]^3 frame steps across `border`.  The model ray is rotated into the world and rounded; the coordinate is then
    computed back exactly from those doubles: world to model by the exact inverse rotation, the face's plane, hx = x + 1/2."""
    fwd, back = _mp_rotation(CUBE_AXIS, CUBE_ANGLE), _mp_rotation(CUBE_AXIS, -CUBE_ANGLE)
    h = mpmath.mpf(0.5)
    rungs = []
    for k in LADDER_K:
        for sgn in (1, -1):
            a = mpmath.mpf(border) + sgn * mpmath.mpf(2) ** -k
            o = [float(c) for c in _mp_apply(fwd, [a - h, mpmath.mpf(1.5), mpmath.mpf(other) - h])]
            d = [float(c) for c in _mp_apply(fwd, [mpmath.mpf(0), mpmath.mpf(-1), mpmath.mpf(0)])]
            om, dm = _mp_apply(back, mp_vec(o)), _mp_apply(back, mp_vec(d))
            t = (h - om[1]) / dm[1]
            hx, hz = om[0] + t * dm[0] + h, om[2] + t * dm[2] + h
            rungs.append(Rung(o, d, hx, hz, decide(hx, border), 1 if hx > border else -1))
    return rungs


def ladder_expectation(rungs, colour_at, border, which=0):
    """Per rung the set of allowed colours: the reference's colour at the exact coordinate for a decided rung, else either of the two
    colours that meet at the border.  The held coordinate is far from its own borders (asserted: 1e-3 either way changes nothing), so
    its rounding to a double decides nothing."""
    out = []
    eps = 2.0 ** -30
    for r in rungs:
        other = float(r.other)
        def at(c, shift=0.0):
            return colour_at(c, other + shift) if which == 0 else colour_at(other + shift, c)
        for probe in (border - 0.01, border + 0.01):
            assert at(probe, -1e-3) == at(probe) == at(probe, 1e-3), "the held coordinate sits on a border of its own"
        if r.decided:
            out.append({at(float(r.coord))})
        else:
            out.append({at(border - eps), at(border + eps)})
    return out


def undecided_share(rungs):
    return sum(not r.decided for r in rungs) / len(rungs)

"""A bit-exact reference for the triangle test, and the rays and meshes of tests/test_triangle_borders.py.

The reference restates Triangle.fs:43-66 operation by operation, in the text's order and without early rejects: once in plain Python
floats (`tri_reference`), once elementwise in numpy float64 over rays x triangles (`tri_reference_grid`: every numpy operation is one
IEEE operation, nothing is fused).  It shares nothing with the oracle or the device.

Why plain floats can be the expectation bit for bit.  edge1, edge2 and s are single subtractions.  If every product and every partial
sum of h = d x edge2, a = edge1 . h, sh = s . h, q = s x edge1, dq = d . q and tn = edge2 . q is exactly representable in binary64, then
a, sh, dq and tn are the same numbers in every correct evaluation, with or without fused multiply-adds, and what is left - 1 / a, f * sh,
f * dq, u + v, f * tn - are single correctly rounded operations.  `exact_guard` checks exactly that over fractions.Fraction;
`lattice_guard` checks the same for the lattice families in int64 (all their inputs are integers over one power of two) for every ray
against every triangle at once.  Every ray of every family is constructed to pass; a test asserts that none is dropped.

The lattice camera.  fov_y = nextafter(2 atan(1/2), +inf) has tan(fov_y / 2) == 0.5 exactly; with look_at = o + (0, 0, -1), up = (0, 1, 0),
aspect 2 and a 65 x 33 frame the image plane is i = (-1, 0, 0), j = (0, 1, 0), k = (0, 0, -1), pixel_width = 1/16, pixel_height = 1/64
(Image.fs:71-72 takes res_h - 1 for the height and res_v - 1 for the width), top_left = (-31/32, 63/128): the ray of pixel (x, y) under
a dyadic sample offset (ox, oy) has d = (31/32 - (x + ox) / 16, 63/128 - (y - oy) / 64, -1), exactly.

slightOffset.  A frame's geometry ray starts at o + 0.0001 d (Shading.fs:129), which is no dyadic number.  So the frames and AOV planes
of the exact families are taken by a camera at BIG = 2^42 + 16 on every axis: there half an ulp is 2^-11 = 4.9e-4 > 1e-4 |d_c| (|d_x| reaches
3.03), the offset is absorbed whether the sum is fused or not (asserted), and the ray the device traces starts at o itself.  Mesh
vertices are o + t d with t a multiple of 1/8 along the rays of even pixels: multiples of 2^-10, representable beside 2^42, and every
difference the triangle test forms is a small dyadic number again.  Explicit rays (`closest`, `blocked`) carry no offset and use a camera near the origin as well."""
import functools
import math
from fractions import Fraction as F

import numpy as np

import functracer_amd as ft

EPS = 0.0000001                                                     # Triangle.fs:44
REJECT = 1.000000000000004                                          # tri_hit's division-free bound (ft_kernels.hip)

# ---------------------------------------------------------------------------------------------------------------- the reference


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def tri_reference(T, o, d):
    """Triangle.fs:43-66 in Python floats.  T = (vertex0, vertex1, vertex2).  Returns (hit, t, u, v); what the text never computes is None."""
    T = [tuple(float(c) for c in p) for p in T]
    o, d = tuple(float(c) for c in o), tuple(float(c) for c in d)
    edge1 = _sub(T[1], T[0])
    edge2 = _sub(T[2], T[0])
    h = _cross(d, edge2)
    a = _dot(edge1, h)
    if a > -EPS and a < EPS:
        return False, None, None, None
    f = 1.0 / a
    s = _sub(o, T[0])
    u = f * _dot(s, h)
    if u < 0.0 or u > 1.0:
        return False, None, u, None
    q = _cross(s, edge1)
    v = f * _dot(d, q)
    if v < 0.0 or u + v > 1.0:
        return False, None, u, v
    t = f * _dot(edge2, q)
    if t > EPS:
        return True, t, u, v
    return False, t, u, v


def tri_reference_grid(tris, o, d, chunk=512):
    """The same for rays o, d [m, 3] against triangles tris [n, 3, 3]: (hit [m, n] bool, t [m, n], inf where no hit)."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    v0 = tris[:, 0]
    e1, e2 = tris[:, 1] - v0, tris[:, 2] - v0
    hit_all, t_all = np.zeros((o.shape[0], tris.shape[0]), dtype=bool), np.full((o.shape[0], tris.shape[0]), np.inf)
    X, Y, Z = 0, 1, 2
    for lo in range(0, o.shape[0], chunk):
        O, D = o[lo:lo + chunk, None, :], d[lo:lo + chunk, None, :]
        E1, E2 = e1[None], e2[None]
        h = [D[..., Y] * E2[..., Z] - D[..., Z] * E2[..., Y], D[..., Z] * E2[..., X] - D[..., X] * E2[..., Z], D[..., X] * E2[..., Y] - D[..., Y] * E2[..., X]]
        a = E1[..., X] * h[X] + E1[..., Y] * h[Y] + E1[..., Z] * h[Z]
        s = [O[..., k] - v0[None, :, k] for k in range(3)]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            f = 1.0 / a
            u = f * (s[X] * h[X] + s[Y] * h[Y] + s[Z] * h[Z])
            q = [s[Y] * E1[..., Z] - s[Z] * E1[..., Y], s[Z] * E1[..., X] - s[X] * E1[..., Z], s[X] * E1[..., Y] - s[Y] * E1[..., X]]
            v = f * (D[..., X] * q[X] + D[..., Y] * q[Y] + D[..., Z] * q[Z])
            t = f * (E2[..., X] * q[X] + E2[..., Y] * q[Y] + E2[..., Z] * q[Z])
            ok = ~((a > -EPS) & (a < EPS)) & ~((u < 0.0) | (u > 1.0)) & ~((v < 0.0) | (u + v > 1.0)) & (t > EPS)
        hit_all[lo:lo + chunk] = ok
        t_all[lo:lo + chunk] = np.where(ok, t, np.inf)
    return hit_all, t_all


def closest_reference(hit, t):
    """Scene.fs:112-116 over a triangle list: the smallest computed t (t > EPS, so t >= 0), the first in list order among equals
    (np.argmin returns the first minimum).  (hit [m] bool, t [m] with inf for a miss, winner [m] with -1 for a miss)."""
    tt = np.where(hit, t, np.inf)
    win = np.argmin(tt, axis=1)
    best = tt[np.arange(tt.shape[0]), win]
    any_hit = hit.any(axis=1)
    return any_hit, best, np.where(any_hit, win, -1)


def blocked_reference(hit, t, max_dist):
    """Scene.fs:119-121: some triangle has a hit with t < max_dist."""
    return (hit & (t < np.asarray(max_dist, dtype=np.float64)[:, None])).any(axis=1)


# ---------------------------------------------------------------------------------------------------------------- the guards
def representable(x):
    """x (a Fraction) is a binary64 number."""
    try:
        return F(float(x)) == x
    except OverflowError:
        return False


def exact_guard(T, o, d):
    """Every product, every partial sum (in either association) and a, sh, dq, tn of Triangle.fs:43-66 are binary64 numbers."""
    T = [tuple(float(c) for c in p) for p in T]
    o, d = tuple(float(c) for c in o), tuple(float(c) for c in d)
    fr = lambda vec: tuple(F(c) for c in vec)
    e1, e2, s, D = fr(_sub(T[1], T[0])), fr(_sub(T[2], T[0])), fr(_sub(o, T[0])), fr(d)   # single subtractions: the same everywhere

    def cross(a, b):
        out = []
        for i, j in ((1, 2), (2, 0), (0, 1)):
            p, q = a[i] * b[j], a[j] * b[i]
            if not (representable(p) and representable(q) and representable(p - q)):
                return None
            out.append(p - q)
        return tuple(out)

    def dot(a, b):
        p = [a[k] * b[k] for k in range(3)]
        sums = [p[0] + p[1], p[1] + p[2], p[0] + p[2], p[0] + p[1] + p[2]]
        return sums[3] if all(representable(x) for x in p + sums) else None

    h = cross(D, e2)
    if h is None or dot(e1, h) is None or dot(s, h) is None:
        return False
    q = cross(s, e1)
    return q is not None and dot(D, q) is not None and dot(e2, q) is not None


LIMIT = 2 ** 53


def lattice_guard(tris_i, o_i, d_i, chunk=1024):
    """lattice_guard_chunk over all rays, `chunk` at a time."""
    parts = [lattice_guard_chunk(tris_i, o_i[lo:lo + chunk], d_i[lo:lo + chunk]) for lo in range(0, len(o_i), chunk)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(5))


def lattice_guard_chunk(tris_i, o_i, d_i):
    """The guard for integer inputs (coordinates over one power of two): tris_i [n, 3, 3], o_i [m, 3], d_i [m, 3] int64.  Every product
    and every partial sum is formed exactly in int64 and must stay below 2^53 in magnitude (an integer below 2^53 over a power of two
    is a binary64 number).  Returns (kept [m, n] bool, a, sh, dq, tn as exact int64 [m, n])."""
    tris_i, o_i, d_i = (np.asarray(v, dtype=np.int64) for v in (tris_i, o_i, d_i))
    v0 = tris_i[:, 0]
    e1, e2 = (tris_i[:, 1] - v0)[None], (tris_i[:, 2] - v0)[None]
    s = o_i[:, None, :] - v0[None]
    D = d_i[:, None, :]
    worst = np.zeros((o_i.shape[0], tris_i.shape[0]), dtype=np.int64)

    def see(*vals):
        nonlocal worst
        for x in vals:
            worst = np.maximum(worst, np.abs(x))

    def cross(a, b):
        out = []
        for i, j in ((1, 2), (2, 0), (0, 1)):
            p, q = a[..., i] * b[..., j], a[..., j] * b[..., i]
            see(p, q, p - q)
            out.append(p - q)
        return np.stack(np.broadcast_arrays(*out), axis=-1)

    def dot(a, b):
        p = [a[..., k] * b[..., k] for k in range(3)]
        see(*p, p[0] + p[1], p[1] + p[2], p[0] + p[2], p[0] + p[1] + p[2])
        return p[0] + p[1] + p[2]

    for x in (e1, e2, s, D):
        assert np.abs(x).max() < 2 ** 20, "the int64 products below could overflow"
    h = cross(D, e2)
    a, sh = dot(e1, h), dot(s, h)
    q = cross(s, e1)
    dq, tn = dot(D, q), dot(e2, q)
    return worst < LIMIT, a, sh, dq, tn


# ---------------------------------------------------------------------------------------------------------------- the lattice camera
FOV = math.nextafter(2.0 * math.atan(0.5), math.inf)
RES_H, RES_V = 65, 33
TILES = [(0, 0, 64, 32)]
TLX, TLY, PW, PH = F(-31, 32), F(63, 128), F(1, 16), F(1, 64)
# the second has a pixel column with jx == 0 (x = 15) and a pixel row with jy == 0 (y = 31): d = (0, 0, -1) at pixel (15, 31)
OFFSETS = [(0.0, 0.0), (0.5, -0.5), (0.25, -0.5), (-0.25, 0.25)]
NEAR = (F(1, 4), F(-1, 2), F(1))                                     # a camera near the origin, for explicit rays
BIG = (F(2 ** 42 + 16),) * 3                                          # the camera of the frames: slightOffset is absorbed
SLIGHT = 0.0001                                                      # Shading.fs:129
D_SCALE, V_SCALE = 2 ** 8, 2 ** 12                                   # directions are multiples of 1/256, vertices minus the eye of 1/4096


def camera(eye):
    e = [float(c) for c in eye]
    return ft.make_camera(tuple(e), (e[0], e[1], e[2] - 1.0), (0, 1, 0), FOV, 2.0)


def pixel_dir(x, y, ox=0.0, oy=0.0):
    """The exact direction of pixel (x, y) under the sample offset (ox, oy) (Image.fs:83-89 with the plane above)."""
    jx, jy = TLX + (x + F(ox)) * PW, TLY - (y - F(oy)) * PH
    return (-jx, jy, F(-1))


def tile_pixels():
    return [(x, y) for (x0, y0, w, h) in TILES for y in range(y0, y0 + h) for x in range(x0, x0 + w)]


@functools.lru_cache(maxsize=None)
def lattice_rays(eye_name):
    """Every tile pixel under every offset of OFFSETS: (o [m, 3], d [m, 3] float64, d_i [m, 3] int64 = d * D_SCALE, xs, ys, offset index)."""
    eye = {"near": NEAR, "big": BIG}[eye_name]
    px = tile_pixels()
    d, xs, ys, ks = [], [], [], []
    for k, (ox, oy) in enumerate(OFFSETS):
        for x, y in px:
            d.append(pixel_dir(x, y, ox, oy))
            xs.append(x), ys.append(y), ks.append(k)
    d_i = np.array([[int(c * D_SCALE) for c in v] for v in d], dtype=np.int64)
    assert all(F(int(c), D_SCALE) == e for row, v in zip(d_i, d) for c, e in zip(row, v))
    df = d_i.astype(np.float64) / D_SCALE
    o = np.broadcast_to(np.array([float(c) for c in eye]), df.shape).copy()
    out = (o, df, d_i, np.array(xs), np.array(ys), np.array(ks))
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- Family A: lattice meshes
# A mesh is kept relative to the eye: rel [n, 3, 3] as exact Fractions' integers over V_SCALE.  vertices(rel, eye) adds the eye.
T_SHEET = [F(2), F(5, 2), F(9, 4), F(3)]                            # neighbouring vertices lie at different depths: tilted triangles
T_FLAT = [F(5, 2), F(21, 8), F(11, 4), F(5, 2)]                    # the gapped mesh of the BSP depths: shallow tilt (see gapped())


def _vertex(gx, gy, t):
    """The vertex at depth t along the ray of pixel (gx, gy), minus the eye, in units of 1 / V_SCALE."""
    v = [t * c * V_SCALE for c in pixel_dir(gx, gy)]
    assert all(c.denominator == 1 for c in v), (gx, gy, t)
    return tuple(int(c) for c in v)


def _grid(x0, x1, y0, y1, ts, keep=None):
    """Triangles over the vertex grid at the even pixels of [x0, x1] x [y0, y1], vertex (a, b) at depth ts[(a + 2 b) % 4] along its pixel's
    ray; the quads' diagonals alternate (hubs of 4 and 8 triangles), and so does the winding.  keep(cell) filters quads."""
    out, n = [], 0
    at = lambda a, b: _vertex(x0 + 2 * a, y0 + 2 * b, ts[(a + 2 * b) % 4])
    for b in range((y1 - y0) // 2):
        for a in range((x1 - x0) // 2):
            if keep is not None and not keep(a, b):
                continue
            p00, p10, p01, p11 = at(a, b), at(a + 1, b), at(a, b + 1), at(a + 1, b + 1)
            pair = [(p00, p10, p11), (p00, p11, p01)] if (a + b) % 2 == 0 else [(p00, p10, p01), (p10, p11, p01)]
            for tri in pair:
                out.append(tri if n % 2 == 0 else (tri[0], tri[2], tri[1]))
                n += 1
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def sheet():
    """24 x 12 quads, 576 triangles over pixels 8 .. 56 x 4 .. 28: the rim runs through pixel centres, pixel columns 7 and 57 and pixel rows
    3 and 29 pass one pixel outside it."""
    return _grid(8, 56, 4, 28, T_SHEET)


@functools.lru_cache(maxsize=None)
def duplicates():
    """Every triangle of a coarser sheet twice, the copies next to each other in the list: the first must win, on every ray."""
    g = _grid(12, 52, 6, 26, T_SHEET)
    return np.repeat(g, 2, axis=0)


@functools.lru_cache(maxsize=None)
def fan():
    """Eight triangles around a hub on the ray of pixel (32, 16), the rim at alternating depths, the winding alternating."""
    hub = _vertex(32, 16, F(5, 2))
    ring = [(6, 0), (6, 6), (0, 6), (-6, 6), (-6, 0), (-6, -6), (0, -6), (6, -6)]
    rim = [_vertex(32 + dx, 16 + dy, F(2) if k % 2 == 0 else F(3)) for k, (dx, dy) in enumerate(ring)]
    out = []
    for k in range(8):
        tri = (hub, rim[k], rim[(k + 1) % 8])
        out.append(tri if k % 2 == 0 else (tri[0], tri[2], tri[1]))
    return np.array(out, dtype=np.int64)


def _bounds_cut(tris):
    """BspMesh.compile's cut of a triangle set: (axis, twice the plane's position) - the middle of the longest axis of the bounds."""
    p = tris.reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))                                   # the first of equal extents, as the comparisons of the text give it
    return axis, int(lo[axis] + hi[axis])


def _gap(tris, depth):
    """Remove every triangle that touches or straddles the cut of its set, then recurse into the two sides: nothing is left to clip."""
    if depth == 0 or len(tris) < 2:
        return tris
    axis, twice = _bounds_cut(tris)
    c = 2 * tris[:, :, axis]
    above, below = (c > twice).all(axis=1), (c < twice).all(axis=1)
    return np.concatenate([_gap(tris[above], depth - 1), _gap(tris[below], depth - 1)])


@functools.lru_cache(maxsize=None)
def gapped(depth):
    """The sheet at a shallow tilt with every quad removed that BspMesh.compile would cut at the first `depth` levels.  Whether the
    builder then really clips nothing is for a test to say (the tree's triangle records against the input's, bit for bit)."""
    return _gap(_grid(4, 60, 2, 30, T_FLAT), depth)


MESHES = {"sheet": sheet, "duplicates": duplicates, "fan": fan}
BSP_DEPTHS = (1, 2, 3)


def vertices(rel, eye, ops=None):
    """The float vertices [n, 9] of a mesh at `eye`, every coordinate checked to be exact; with `ops` (a per-axis scale, then a translation)
    the vertices in the frame under that transform."""
    out = np.zeros(rel.shape, dtype=np.float64)
    s, tr = ((F(1),) * 3, (F(0),) * 3) if ops is None else (tuple(F(c) for c in ops[0][1]), tuple(F(c) for c in ops[1][1]))
    for idx in np.ndindex(rel.shape):
        exact = (F(int(rel[idx]), V_SCALE) + eye[idx[2]] - tr[idx[2]]) / s[idx[2]]
        assert representable(exact), (idx, exact)
        out[idx] = float(exact)
    return out.reshape(-1, 9)


def transform_ops(eye):
    """Power-of-two scales and a dyadic translation that carries the eye's magnitude: the model frame is small whatever the eye."""
    return [("scale", (2.0, 0.5, 4.0)), ("translate", tuple(float(e + c) for e, c in zip(eye, (F(1, 2), F(-1, 4), F(-1)))))]


@functools.lru_cache(maxsize=None)
def lattice_answers(mesh, eye_name):
    """The reference's answers for a mesh (a name of MESHES or ("gapped", depth)) on lattice_rays(eye_name), computed once and shared:
    a dict of hit, t, winner [m], the whole hit / t grids and the guard's verdict.  The triangle test only sees differences to the eye,
    which are the same small numbers for both eyes - the floats are formed from the eye all the same."""
    rel = gapped(mesh[1]) if isinstance(mesh, tuple) else MESHES[mesh]()
    eye = {"near": NEAR, "big": BIG}[eye_name]
    o, d, d_i, xs, ys, ks = lattice_rays(eye_name)
    tris = vertices(rel, eye)
    hit, t = tri_reference_grid(tris, o, d)
    kept, a, sh, dq, tn = lattice_guard(rel, np.zeros_like(d_i), d_i)
    any_hit, best, win = closest_reference(hit, t)
    out = {"rel": rel, "tris": tris, "hit_grid": hit, "t_grid": t, "hit": any_hit, "t": best, "winner": win, "kept": kept, "exact": (a, sh, dq, tn)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def as_planes(values, xs, ys, ks, fill):
    """Per-ray values as one [RES_V, RES_H] plane per offset."""
    out = [np.full((RES_V, RES_H), fill, dtype=np.asarray(values).dtype) for _ in OFFSETS]
    for k in range(len(OFFSETS)):
        m = ks == k
        out[k][ys[m], xs[m]] = np.asarray(values)[m]
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
COLOUR = (0.9, 0.5, 0.2)
LIGHT = (-1.0, -1.3, -0.8)
FAR_SPHERE = [("scale", (0.25, 0.25, 0.25)), ("translate", (300.0, 40.0, 500.0))]   # behind the cameras, off every ray


def _far(b, eye):
    ops = [FAR_SPHERE[0], ("translate", tuple(float(e) + c for e, c in zip(eye, FAR_SPHERE[1][1])))]
    return b.material(b.transform(ops, b.primitive(ft.SPHERE)), colour=(0.1, 0.2, 0.9))


def lower_mesh(tris, depth=0, ops=None, eye=NEAR, beside=False, floor=False, light=True):
    """lower(builder): one `bspMesh depth` of tris [n, 9] (under `ops`); beside: a far sphere as a second item (the generic k_primary);
    floor: a plane 4 below the eye; light: one directional light."""
    def lower(b):
        b.clear()
        node = b.bsp_mesh(depth, np.asarray(tris).reshape(-1, 9))
        if ops:
            node = b.transform(list(ops), node)
        items = [b.material(node, colour=COLOUR)]
        if beside:
            items.append(_far(b, eye))
        if floor:
            items.append(b.material(b.translate((0.0, float(eye[1]) - 4.0, 0.0), b.primitive(ft.PLANE)), colour=(0.4, 0.8, 0.4)))
        b.set_objects(b.group(items))
        if light:
            b.add_directional(LIGHT, (1, 1, 1))
        b.commit()
    return lower


def index_colour(i):
    """A colour that names a triangle: three base-64 digits over 64, exact in binary64."""
    return ((i % 64) / 64.0, ((i // 64) % 64) / 64.0, (i // 4096) / 64.0 + 1.0 / 128.0)


def colour_index(col):
    c = np.asarray(col)
    return (np.rint(c[..., 0] * 64) + 64 * np.rint(c[..., 1] * 64) + 4096 * np.rint((c[..., 2] - 1.0 / 128.0) * 64)).astype(np.int64)


def lower_group(tris):
    """lower(builder): the triangles as a group of `triangle` primitives, each under a material whose colour is its list index."""
    def lower(b):
        b.clear()
        t = np.asarray(tris).reshape(-1, 3, 3)
        b.set_objects(b.group([b.material(b.triangle(tuple(p[0]), tuple(p[1]), tuple(p[2])), colour=index_colour(i)) for i, p in enumerate(t)]))
        b.commit()
    return lower


def lower_csg(tris, depth=0, eye=NEAR):
    """lower(builder): union(mesh, far sphere) - the mesh's hits go through the hit lists of a CSG node, which scan the list in order."""
    def lower(b):
        b.clear()
        mesh = b.material(b.bsp_mesh(depth, np.asarray(tris).reshape(-1, 9)), colour=COLOUR)
        b.set_objects(b.group([b.union(mesh, _far(b, eye))]))
        b.commit()
    return lower


# ---------------------------------------------------------------------------------------------------------------- Family B: the ulp band
def step(x, k):
    """x moved by k doubles."""
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


K_RANGE = range(-8, 25)
B_SIZES = [3.0, 0.7000000000000042, 1.7000000000000002, 3.900000000000001]   # 53-bit, no powers of two; the first doubles from 3, 0.7, 1.7 and 3.9 on that meet the band conditions (asserted)
B_FRAMES = [(1.0, -1.0), (0.5, -2.0)]                                # (B, dz): powers of two


def band_triangle(A, B, axis, flip):
    """v0 at the origin, the 53-bit edge A along `axis` (0: edge1 = (A, 0, 0), edge2 = (0, B, 0); 1: edge1 = (B, 0, 0), edge2 = (0, A, 0));
    flip swaps vertex1 and vertex2 (a changes sign, u and v change roles)."""
    v1, v2 = ((A, 0.0, 0.0), (0.0, B, 0.0)) if axis == 0 else ((B, 0.0, 0.0), (0.0, A, 0.0))
    return ((0.0, 0.0, 0.0), v2, v1) if flip else ((0.0, 0.0, 0.0), v1, v2)


def band_cases(A):
    """(label, T, o, d, k) over the borders u (or v) = 1, = 0, the hypotenuse, for both axes, windings and frames, k in K_RANGE.  The
    coordinate along the A edge is stepped double by double; the other is 0, B / 4 or B / 2 (times a power of two: exact products)."""
    out = []
    for B, dz in B_FRAMES:
        for axis in (0, 1):
            for flip in (False, True):
                T = band_triangle(A, B, axis, flip)
                for border in ("one", "zero", "zero_tiny", "hyp"):
                    for k in K_RANGE:
                        if border == "one":
                            ca, cb = step(A, k), 0.0
                        elif border == "zero":
                            ca, cb = k * 2.0 ** -200, B / 4
                        elif border == "zero_tiny":
                            ca, cb = k * (5e-324 if B == 1.0 else 2.0 ** -1000), B / 4   # subnormals where no product leaves them (B == 1)
                        else:
                            ca, cb = step(A / 2, k), B / 2
                        o = (ca, cb, 1.0) if axis == 0 else (cb, ca, 1.0)
                        out.append((f"{border}/B={B}/axis={axis}/flip={int(flip)}", T, o, (0.0, 0.0, dz), k))
    return out


# ---------------------------------------------------------------------------------------------------------------- Family C: epsilon borders
def eps_cases():
    """(label, T, o, d, max_dists or None).  a = A B for d = (0, 0, -1); t = f * (A B sz)."""
    P, N = math.nextafter(EPS, 0.0), math.nextafter(EPS, 1.0)
    out = []
    for name, A in (("pred", P), ("eps", EPS), ("succ", N)):       # |a| on the near-parallel border: rejected only inside the open interval
        for flip in (False, True):
            T = band_triangle(A, 1.0, 0, flip)
            inside = (A / 2, 0.25, 1.0)
            out.append((f"a={'-' if flip else ''}{name}", T, inside, (0.0, 0.0, -1.0), None))
    for e in range(-24, 25, 2):                                      # the same triangle and ray, d scaled: the reject depends on |d|
        T = band_triangle(0.7, 2.0 ** -10, 0, False)
        out.append((f"d*2^{e}", T, (0.25, 2.0 ** -12, 2.0 ** e), (0.0, 0.0, -(2.0 ** e)), None))   # t = 1 throughout
        T = band_triangle(3.0, 2.0 ** -12, 1, True)
        out.append((f"d*2^{e}/flip", T, (2.0 ** -14, 0.5, 2.0 ** e), (0.0, 0.0, -(2.0 ** e)), None))
    T = band_triangle(1.0, 1.0, 0, False)                            # a = 1: t = tn = sz exactly
    for name, z in (("pred", P), ("eps", EPS), ("succ", N), ("behind", -1.0), ("at", 0.0)):
        out.append((f"t={name}", T, (0.25, 0.25, z), (0.0, 0.0, -1.0), None))
    for z in (1.0, 3.0, 0.7):                                        # max_dist on the border of t < max_dist
        out.append((f"max_dist/t={z}", T, (0.25, 0.25, z), (0.0, 0.0, -1.0), (math.nextafter(z, 0.0), z, math.nextafter(z, math.inf), 1e300)))
    return out


DEGENERATE = [((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0)),   # collinear: a == 0 for every ray
              ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))]     # a good one in the same plane, after it in the list
# far triangles that bring a small mesh up to the 8 a tree needs (bvh_for_leaf, ft_scene.cpp); dyadic, beside every ray of the families
FILLER = [((64.0 + 2 * k, 64.0, -8.0), (65.0 + 2 * k, 64.0, -8.0), (64.0 + 2 * k, 65.0, -8.0)) for k in range(8)]


def with_filler(tris):
    return np.array([np.array(t, dtype=np.float64).reshape(9) for t in list(tris) + FILLER])

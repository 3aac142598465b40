"""Scene builders for tests/test_device_limits.py: scenes at the documented limits of the device path and one past
each.  Every scene is data or a function of a builder, so that the oracle, a host-only context and the device build the same one.

CSG trees are nested tuples:
    ("prim", kind, ops, i)      a primitive under `ops` with the material colour of leaf i (still a bare primitive for the flattener)
    ("group", [tree, ...])      a group
    ("tris", [[a, b, c], ...], i)   a group of bare triangles (one brute-force triangle list on the device)
    ("mesh", tris, i)           bspMesh 0
    ("xf", ops, tree)           a transform
    ("csg", op, A, B)
"""
import numpy as np

import functracer_amd as ft

OPS = [ft.UNION, ft.INTERSECT, ft.SUBTRACT, ft.EXCLUDE]


def leaf_colour(i):
    """Pairwise distinct in every channel and exact in binary: a hit's material colour names its leaf."""
    return (0.25 + i / 64.0, 0.75 - i / 128.0, 0.125 + i / 256.0)


def build_tree(b, tree, no_csg=False):
    """no_csg: every CSG node becomes a group of its operands - the same surfaces, none merged, none flipped."""
    kind = tree[0]
    if kind == "prim":
        n = b.primitive(tree[1])
        if tree[2]:
            n = b.transform(list(tree[2]), n)
        return b.material(n, colour=leaf_colour(tree[3]))
    if kind == "group":
        return b.group([build_tree(b, t, no_csg) for t in tree[1]])
    if kind == "tris":
        return b.material(b.group([b.triangle(*t) for t in tree[1]]), colour=leaf_colour(tree[2]))
    if kind == "mesh":
        return b.material(b.bsp_mesh(0, np.asarray(tree[1], dtype=np.float64).reshape(-1, 9)), colour=leaf_colour(tree[2]))
    if kind == "xf":
        return b.transform(list(tree[1]), build_tree(b, tree[2], no_csg))
    assert kind == "csg"
    if no_csg:
        return b.group([build_tree(b, tree[2], True), build_tree(b, tree[3], True)])
    return b.csg(tree[1], build_tree(b, tree[2]), build_tree(b, tree[3]))


def is_bare(tree):
    """ft_scene.cpp, bare_primitive: a primitive under single-child scene functions."""
    return tree[0] == "prim" or (tree[0] == "xf" and is_bare(tree[2]))


def tree_facts(tree):
    """What a tree is by construction: its CSG depth, the (level, op) pairs it holds (levels from 1), the most list marks live at once
    (two per open CSG that is not a fused pair: one before A, one more before B), the most marks live when an OP_SKIP_IF_EMPTY is
    reached (its own A mark included), the most marks under a fused pair, and the leaves inside the B operand of a CSG at level 5 or
    deeper ("deep" leaves)."""
    facts = {"depth": 0, "ops": set(), "marks": 0, "marks_at_skip": 0, "marks_under_pair": -1, "deep": set(), "leaves": set()}

    def walk(t, level, marks, deep):
        k = t[0]
        if k == "csg":
            lv = level + 1
            facts["depth"] = max(facts["depth"], lv)
            facts["ops"].add((lv, t[1]))
            if is_bare(t[2]) and is_bare(t[3]):                       # OP_CSG_PAIR: no marks of its own
                facts["marks_under_pair"] = max(facts["marks_under_pair"], marks)
                walk(t[2], lv, marks, deep); walk(t[3], lv, marks, deep or lv >= 5)
                return
            walk(t[2], lv, marks + 1, deep)
            facts["marks"] = max(facts["marks"], marks + 1)
            if t[1] in (ft.SUBTRACT, ft.INTERSECT):
                facts["marks_at_skip"] = max(facts["marks_at_skip"], marks + 1)
            facts["marks"] = max(facts["marks"], marks + 2)
            walk(t[3], lv, marks + 2, deep or lv >= 5)
        elif k == "group":
            for c in t[1]:
                walk(c, level, marks, deep)
        elif k == "xf":
            walk(t[2], level, marks, deep)
        else:
            i = t[-1]
            facts["leaves"].add(i)
            if deep:
                facts["deep"].add(i)
    walk(tree, 0, 0, False)
    return facts


# -------------------------------------------------------------------------------------------------------------------------------
# 1. CSG chains.  The operands stand around a common centre, each pushed 0.8 along its own direction, alternately a sphere and a
# cube: every operand's surface cuts through every other operand, so that whatever subtract and intersect leave of the outer operands
# is bounded by surfaces of the inner ones, and a ray through the middle crosses 2 to 10 surviving surfaces.

def _direction(k):
    z = 1.0 - 2.0 * ((k * 0.618033988749895 + 0.3) % 1.0)
    a = 2.399963229728653 * k
    return np.array([np.sqrt(1 - z * z) * np.cos(a), z, np.sqrt(1 - z * z) * np.sin(a)])


def _operand(k, i, small=False):
    c = tuple(0.45 * _direction(k) + (0.2, 0.0, 0.2))
    if small:
        c = tuple(0.9 * _direction(k) + (0.2, 0.0, 0.2))
    if k % 2 == 0:
        return ("prim", ft.SPHERE, [("scale", 0.65 if small else 1.05), ("translate", c)], i)
    return ("prim", ft.CUBE, [("scale", (1.1, 1.2, 1.0) if small else (1.7, 1.9, 1.6)), ("rotate", (0.3, 1.0, 0.2), 0.4 + 0.1 * k), ("translate", c)], i)


def _small_tris(i):
    """Four bare triangles forming an open tent over the middle."""
    a, b, c, d, top = (-0.9, -0.7, -0.9), (1.1, -0.7, -0.9), (1.1, -0.7, 1.1), (-0.9, -0.7, 1.1), (0.1, 1.1, 0.1)
    return ("tris", [[a, b, top], [b, c, top], [c, d, top], [d, a, top]], i)


def _small_mesh(i):
    """bspMesh 0 of an octahedron (8 triangles: enough for the device BVH) around the middle."""
    c = np.array([0.3, 0.1, 0.1])
    v = [c + 1.0 * np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return ("mesh", [[*v[a], *v[b], *v[c]] for a, b, c in f], i)


def right_deep(depth, shift, innermost, pair_levels=()):
    """A op (A op (A op ... (A op X))): every B operand is a CSG, so 2 marks stay live per level.  `innermost` is X: anything but a
    bare primitive keeps the last level from fusing into OP_CSG_PAIR, so that depth 8 holds 16 marks.  The operator of level k
    (from 1) is OPS[(k - 1 + shift) % 4].  pair_levels: levels whose A operand is itself a fused pair of two small primitives."""
    leaf = [0]

    def nxt():
        leaf[0] += 1
        return leaf[0] - 1

    def level(k):
        # A small A under union and exclude, or it would hide what lies deeper; and a small A at level 6, which whole waves miss
        # (OP_SKIP_IF_EMPTY then fires under 11 marks)
        small = OPS[(k - 1 + shift) % 4] in (ft.UNION, ft.EXCLUDE) or k == 6
        if k in pair_levels and k < 8:
            # (an unrotated cube at levels 5 and 7: an axis-parallel ray meets faces at its origin and the pair takes the generic route)
            a = ("csg", ft.UNION, _operand(k - 1, nxt(), True), ("prim", ft.SPHERE if k == 6 else ft.CUBE, [("scale", 0.8), ("translate", tuple(0.7 * _direction(k + 9)))], nxt()))
        else:
            a = _operand(k - 1, nxt(), small)
        if k == depth:
            b = innermost(k, nxt)
        else:
            b = level(k + 1)
        return ("csg", OPS[(k - 1 + shift) % 4], a, b)
    return level(1)


def x_group(k, nxt):
    """A group of two primitives: bare_primitive() stops at a Group node, so the level is not a pair."""
    return ("group", [_operand(k, nxt()), _operand(k + 1, nxt(), True)])


def x_tris(k, nxt):
    """A group of bare triangles: a Group node again, flattened to one brute-force triangle list."""
    return _small_tris(nxt())


def x_mesh(k, nxt):
    """A bspMesh node: bare_primitive() returns false for Mesh."""
    return _small_mesh(nxt())


def x_prim(k, nxt):
    """A bare primitive: the last level fuses into OP_CSG_PAIR, pushing into a list that lies under 2 * (depth - 1) marks."""
    return _operand(k, nxt())


def left_deep(depth, shift):
    """((((X op A) op A) op A) ...): depth + 1 marks at most; X a group, so that the innermost level is no pair."""
    leaf = [0]

    def nxt():
        leaf[0] += 1
        return leaf[0] - 1
    t = ("group", [_operand(0, nxt()), _operand(1, nxt(), True)])
    for k in range(depth, 0, -1):                                   # built inside out: level `depth` first
        t = ("csg", OPS[(k - 1 + shift) % 4], t, _operand(depth + 1 - k, nxt(), k == 3 or OPS[(k - 1 + shift) % 4] in (ft.UNION, ft.EXCLUDE)))
    return t


def mixed(shift):
    """Depth 8, both shapes: the root's A is a left-deep chain of 4 levels that ends in a fused pair, its B a right-deep chain of 7
    that ends in a group: 2 + 14 = 16 marks."""
    leaf = [40]

    def nxt():
        leaf[0] += 1
        return leaf[0] - 1
    a = ("csg", ft.UNION, _operand(0, nxt()), _operand(1, nxt()))
    for k in (4, 3, 2):
        a = ("csg", OPS[(k + shift) % 4], a, _operand(6 - k, nxt(), True))
    return ("csg", OPS[shift % 4], a, right_deep(7, shift + 1, x_group))


def csg_cases():
    """name -> (tree, wrap): wrap(b, node) gives the list of top-level items."""
    plain = lambda b, n: [n]
    under_xf = lambda b, n: [b.transform([("scale", (1.3, 0.7, 1.1)), ("rotate", (1.0, 2.0, 0.5), 0.8), ("translate", (0.2, 0.1, -0.3))], n)]
    beside = lambda b, n: [b.material(b.transform([("scale", 0.6), ("rotate", (0, 1, 0), 0.5), ("translate", (2.4, -0.8, -0.6))], b.primitive(ft.CUBE)), colour=(0.3, 0.9, 0.6)), n,
                           b.material(b.transform([("scale", 0.7), ("translate", (-2.6, 0.3, 1.0))], b.primitive(ft.SPHERE)), colour=(0.9, 0.9, 0.2), reflectance=0.4, shineyness=10)]
    return {
        "right5": (right_deep(5, 0, x_group), plain),
        "right6": (right_deep(6, 1, x_tris), plain),
        "right7": (right_deep(7, 2, x_mesh), plain),
        "right8": (right_deep(8, 2, x_group), plain),
        "right8-shift3": (right_deep(8, 3, x_tris), plain),
        "right8-shift0": (right_deep(8, 0, x_group), plain),
        "right8-shift1": (right_deep(8, 1, x_mesh), plain),
        "right8-shift2-pairs": (right_deep(8, 2, x_prim, pair_levels=(5, 6, 7)), plain),
        "left8": (left_deep(8, 1), plain),
        "mixed8": (mixed(2), plain),
        "right8-transformed": (right_deep(8, 2, x_group), under_xf),
        "right8-beside": (right_deep(8, 1, x_group), beside),
    }


def build_csg_case(b, name, no_csg=False):
    tree, wrap = csg_cases()[name]
    b.clear()
    b.set_objects(b.group(wrap(b, build_tree(b, tree, no_csg))))
    b.add_directional((-0.4, -1.0, 0.6), (1.0, 0.9, 0.8))
    b.add_positional((3.0, 4.0, -5.0), (1.0, 0.02, 0.01), (0.6, 0.7, 1.0))
    b.commit()


def csg_rays(seed):
    """4000 random rays toward the chain and 600 axis-parallel ones (an axis-parallel ray meets cube faces at its origin, Plane.fs:13-16,
    and takes the generic route through OP_CSG_PAIR).  The axis-parallel rays come in 8x8 patches of neighbours, 64 to a wave, so
    that a whole wave misses a small operand."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(4000, 3)) * 3.0
    target = np.array([0.2, 0.0, 0.2]) + rng.normal(size=(4000, 3)) * 0.6
    d = (target - o) * rng.uniform(0.2, 3.0, size=(4000, 1))
    oo, dd = [o], [d]
    g = (np.arange(8) + 0.5) * 0.15
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for patch in range(3):
            base = rng.uniform(-1.3, 0.5, size=2)
            po = np.zeros((64, 3)); pd = np.zeros((64, 3))
            po[:, axis] = -6.0 if patch != 1 else 6.0
            po[:, u] = base[0] + np.repeat(g, 8); po[:, v] = base[1] + np.tile(g, 8)
            pd[:, axis] = (1.5 if patch != 1 else -0.75)
            oo.append(po); dd.append(pd)
    po = np.round(rng.uniform(-2.5, 2.5, size=(24, 3)) * 4) / 4     # origins on face planes of the unrotated cubes of the other top-level items
    pd = np.eye(3)[rng.integers(0, 3, size=24)] * rng.choice([-1.0, 1.0], size=(24, 1))
    oo.append(po); dd.append(pd)
    return np.concatenate(oo), np.concatenate(dd)


def csg_liveness(orc, plain, name, o, d):
    """(share of the rays that hit, share of the hits that are alive) on the oracle alone.  A hit is alive when its normal is flipped
    or its leaf lies inside the B operand of a level >= 5.  The leaf is read from the material colour.  Flipped: `plain` holds the
    same surfaces without any CSG node (build_csg_case(no_csg=True)); the hit is found among ALL of the plain scene's hits on the ray
    by its t, and its normal compared with the plain one."""
    hit, t, _, n, col = orc.closest(o, d)
    m = hit.astype(bool)
    deep = np.array([leaf_colour(i) for i in sorted(tree_facts(csg_cases()[name][0])["deep"])])
    is_deep = (np.abs(col[:, None, :] - deep[None]).max(axis=2) < 1e-12).any(axis=1)
    counts, pt, _, pn = plain.all_hits(o, d, cap=96)
    assert counts.max() <= 96
    valid = np.arange(96)[None, :] < counts[:, None]
    gap = np.where(valid, np.abs(pt - t[:, None]), np.inf)
    gap[~m] = 0.0
    at = gap.argmin(axis=1)
    assert (gap[np.arange(len(o)), at] <= 1e-9 * (1.0 + np.abs(t)))[m].all(), "a CSG hit that is no surface of an operand"
    flipped = np.einsum("ij,ij->i", pn[np.arange(len(o)), at], n) < 0
    return float(m.mean()), float(((is_deep | flipped) & m).sum() / max(1, m.sum()))


CSG_CAMERA = ((1.5, 1.2, -3.4), (0.2, 0.0, 0.2), (0, 1, 0), 42.0)


def onion(b, ops):
    """Concentric spheres of radii 9 .. 1 in a right-deep chain of depth 8: S9 op1 (S8 op2 (... (S2 op8 {S1}))).  The innermost sphere
    sits in a group of one, which keeps level 8 from fusing: 16 marks."""
    b.clear()
    node = b.group([b.primitive(ft.SPHERE)])
    for r, op in zip(range(2, 10), reversed(ops)):
        node = b.csg(op, b.scale(float(r), b.primitive(ft.SPHERE)), node)
    b.set_objects(b.group([node]))
    b.commit()


# -------------------------------------------------------------------------------------------------------------------------------
# 2. A stack of N parallel triangles, 0.1 apart along z.  Triangle i (z = 0.1 i) has the corners (0, 0), (i + 1, 0), (0, 1000): a ray
# along +z at (m + 0.5, 0.5) lies inside it iff (m + 0.5) / (i + 1) + 0.0005 < 1 iff i >= m: it crosses exactly N - m triangles,
# every one at a distance of at least 0.49 from an edge.

STACK_N = 251


def stack_triangles(n=STACK_N):
    return np.array([[0.0, 0.0, 0.1 * i, i + 1.0, 0.0, 0.1 * i, 0.0, 1000.0, 0.1 * i] for i in range(n)])


def crossings(tris, o, d):
    """How many of the triangles each ray crosses at t > 0, by the signed-volume rule in numpy (no tracer involved)."""
    t = np.asarray(tris).reshape(-1, 3, 3)
    count = np.zeros(len(o), dtype=np.int64)
    for a, b, c in t:
        n = np.cross(b - a, c - a)
        den = d @ n
        tt = ((a - o) @ n) / np.where(den == 0, 1.0, den)            # a ray in the triangle's plane crosses nothing
        p = o + tt[:, None] * d
        inside = np.ones(len(o), dtype=bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= np.einsum("ij,j->i", np.cross(v - u, p - u), n) > 0
        count += (den != 0) & (tt > 0) & inside
    return count


def stack_rays(ks, n=STACK_N):
    """One ray per k along +z that crosses exactly k triangles of the stack, then rays that miss it: beside it, and along it."""
    o = [[n - k + 0.5, 0.5, -3.0] for k in ks] + [[n + 0.5, 0.5, -3.0], [-0.5, 0.5, -3.0], [3.5, -0.5, -3.0], [0.5, 0.5, 0.05]]
    d = [[0.0, 0.0, 1.0]] * (len(ks) + 3) + [[1.0, 0.0, 0.0]]
    return np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)


def build_stack(b, n=STACK_N, lit=True):
    """exclude(P1, exclude(exclude(P3, stack), exclude(P2, {}))): exclude keeps every hit of both operands (Csg.fs:46-55), so a lane's
    list really grows to the sum.  P1 a sphere (2 hits), P3 a square and P2 a circle (1 each) lie across the stack's rays in front of
    it; the stack is the B operand at level 3.  With csg_mesh_capacity = n the static capacity is 2 + 1 + n + 1 + 0.  The empty group
    is an operand that can add nothing: its mark is pushed with the list at its longest."""
    b.clear()
    # square: [0, 1]^2 of the plane y = 0 (Cube.fs:9-15); circle: the unit disc.  Centred, stood up across the z axis, scaled, moved.
    big = lambda prim, z, s: b.transform([("translate", (-0.5, 0.0, -0.5) if prim == ft.SQUARE else (0.0, 0.0, 0.0)), ("rotate", (1, 0, 0), np.pi / 2),
                                          ("scale", s), ("translate", (0.0, 0.0, z))], b.primitive(prim))
    p1 = b.material(b.transform([("scale", (400.0, 400.0, 0.5)), ("translate", (0.0, 0.0, -1.5))], b.primitive(ft.SPHERE)), colour=leaf_colour(1))
    p3 = b.material(big(ft.SQUARE, -0.5, 900.0), colour=leaf_colour(3))
    p2 = b.material(big(ft.CIRCLE, 0.1 * n + 0.5, 600.0), colour=leaf_colour(2))
    stack = b.material(b.bsp_mesh(0, stack_triangles(n)), colour=leaf_colour(0))
    node = b.exclude(p1, b.exclude(b.exclude(p3, stack), b.exclude(p2, b.group([]))))
    b.set_objects(b.group([node]))
    if lit:
        b.add_directional((0.2, -0.3, 1.0), (1, 1, 1))
    b.commit()


# -------------------------------------------------------------------------------------------------------------------------------
# 3. Sixteen lights over a plane with one small sphere.

SPHERE_C, SPHERE_R = np.array([0.0, 2.0, 0.0]), 0.2


def light_directions():
    """Sixteen pairwise distinct unit directions, all 45 degrees off the vertical.  Fifteen stand on a ring of azimuths; light 12
    stands 0.125 rad beside light 3, so that their shadows of the sphere overlap."""
    az = np.zeros(16)
    slot = 0
    for l in range(16):
        if l == 12:
            continue
        az[l] = 2 * np.pi * slot / 15 + 0.1
        slot += 1
    az[12] = az[3] + 0.125
    return np.stack([np.sin(np.pi / 4) * np.cos(az), -np.cos(np.pi / 4) * np.ones(16), np.sin(np.pi / 4) * np.sin(az)], axis=1)


def light_colours():
    """Pairwise distinct in every channel, no channel the sum of others at 1e-9."""
    l = np.arange(16)
    return np.stack([0.05 + 0.013 * l + 0.0007 * l * l, 0.04 + 0.011 * ((l * 5) % 16) + 0.0003 * l, 0.03 + 0.009 * ((l * 11) % 16) + 0.0002 * l], axis=1)


def shadow_centre(direction):
    """Where the line through the sphere's centre along a light's direction meets the plane y = 0."""
    return SPHERE_C + direction * (SPHERE_C[1] / -direction[1])


def light_points():
    """P_0 .. P_15 (the sphere blocks light k alone), a point in the open, and one where lights 3 and 12 are both blocked."""
    L = light_directions()
    c = np.array([shadow_centre(v) for v in L])
    pts = c.copy()
    away = (c[3] - c[12]) / np.linalg.norm(c[3] - c[12])
    pts[3] = c[3] + 0.09 * away
    pts[12] = c[12] - 0.09 * away
    both = 0.5 * (c[3] + c[12])
    return np.concatenate([pts, [[0.7, 0.0, -0.9]], [both]])


def blocked_matrix(points, spread=0.0):
    """blocked[i, l]: the segment from points[i] + 1e-4 n toward light l (a half line: the lights are directional) meets the sphere.
    With spread > 0: +1 where every direction within `spread` radians of it does, -1 where none does, 0 in between."""
    L = light_directions()
    o = points + np.array([0.0, 1e-4, 0.0])
    out = np.zeros((len(points), 16), dtype=np.int64)
    for l in range(16):
        d = -L[l]
        w = SPHERE_C - o
        along = w @ d
        dist = np.sqrt(np.maximum(np.einsum("ij,ij->i", w, w) - along ** 2, 0.0))
        if spread == 0.0:
            out[:, l] = (along > 0) & (dist < SPHERE_R)
        else:
            slack = np.linalg.norm(w, axis=1) * np.tan(spread)       # how far a direction within `spread` moves the line at the sphere
            out[:, l] = np.where((along > 0) & (dist + slack < SPHERE_R), 1, np.where(dist - slack > SPHERE_R, -1, 0))
    return out


def expected_colours(blocked):
    """Shading.fs:65-70 over a white plane (normal +y, no specular term at shineyness 0): the sum over the lights that are not blocked
    of colour * (-direction . n), unclamped."""
    L, C = light_directions(), light_colours()
    return ((1 - blocked)[:, :, None] * (C * (-L[:, 1])[:, None])[None]).sum(axis=1)


SOFT = (7, 8, 15)
SOFT_SCATTER = 0.02


def build_lights_scene(b, soft=(), samples=255, n_lights=16, scatter=SOFT_SCATTER):
    b.clear()
    white = dict(colour=(1, 1, 1), roughness=0.0, reflectance=0.0, shineyness=0.0)
    b.set_objects(b.group([b.material(b.primitive(ft.PLANE), **white),
                           b.material(b.transform([("scale", SPHERE_R), ("translate", tuple(SPHERE_C))], b.primitive(ft.SPHERE)), **white)]))
    L, C = light_directions(), light_colours()
    for l in range(n_lights):
        k = l % 16
        if k in soft:
            b.add_soft_directional(tuple(L[k]), samples, scatter, tuple(C[k]))
        else:
            b.add_directional(tuple(L[k]), tuple(C[k]))
    b.commit()


def rays_onto(points, eye=(0.3, 6.0, -0.2)):
    """One ray from the eye to each point; none of them may touch the sphere on its way (asserted)."""
    o = np.tile(np.asarray(eye, dtype=np.float64), (len(points), 1))
    d = points - o
    w = SPHERE_C - o
    along = np.einsum("ij,ij->i", w, d) / np.einsum("ij,ij->i", d, d)
    assert (np.linalg.norm(w - along[:, None] * d, axis=1) > 2 * SPHERE_R).all(), "a view ray passes the sphere too closely"
    return o, d


def build_mixed_lights(b):
    """16 lights - 6 directional, 6 positional, 4 soft, interleaved so that each kind stands on both sides of light 8 - over a plane, a
    CSG item, a reflective sphere and a bspMesh 0."""
    b.clear()
    rng = np.random.default_rng(16)
    csg = b.material(b.subtract(b.primitive(ft.CUBE), b.translate((0.3, 0.4, -0.3), b.scale(0.6, b.primitive(ft.SPHERE)))), colour=(0.8, 0.4, 0.3), shineyness=10)
    mirror = b.material(b.transform([("scale", 0.7), ("translate", (1.8, 0.2, 0.5))], b.primitive(ft.SPHERE)), colour=(0.7, 0.8, 0.9), reflectance=0.5, shineyness=5)
    tent = np.asarray(_small_mesh(0)[1]).reshape(-1, 9)
    mesh = b.material(b.translate((-3.6, 0.3, 0.2), b.bsp_mesh(0, tent)), colour=(0.4, 0.8, 0.4))
    ground = b.material(b.translate((0, -0.5, 0), b.primitive(ft.PLANE)), colour=(0.9, 0.9, 0.9))
    b.set_objects(b.group([ground, csg, mirror, mesh]))
    kinds = "dpsdpdspdpsdpdsp"
    assert kinds.count("d") == 6 and kinds.count("p") == 6 and kinds.count("s") == 4
    for l, k in enumerate(kinds):
        colour = tuple(rng.uniform(0.05, 0.25, size=3))
        direction = tuple(rng.normal(size=3) * 0.6 + (0, -1.5, 0))
        if k == "d":
            b.add_directional(direction, colour)
        elif k == "p":
            b.add_positional(tuple(rng.uniform(-5, 5, size=3) * (1, 0, 1) + (0, 4 + l * 0.2, 0)), (1.0, 0.03, 0.01), colour)
        else:
            b.add_soft_directional(direction, 3 + l, 0.08, colour)
    b.commit()


# -------------------------------------------------------------------------------------------------------------------------------
# 4. Scenes whose reflection tree is alive at 16 levels, with one light.

def build_mirror_hall(b, fancy=False):
    """Two facing mirrors (planes at z = +-3, reflectance 0.9) with a floor and a sphere between them.  fancy: the sphere's shininess
    is above 64, which only the fancy kernel variants shade (ft_flat.h, small_whole_exponent), and it reflects too."""
    b.clear()
    wall = dict(colour=(0.9, 0.85, 0.8), reflectance=0.9, shineyness=0.0)
    back = b.material(b.transform([("rotate", (1, 0, 0), -np.pi / 2), ("translate", (0, 0, 3.0))], b.primitive(ft.PLANE)), **wall)
    front = b.material(b.transform([("rotate", (1, 0, 0), np.pi / 2), ("translate", (0, 0, -3.0))], b.primitive(ft.PLANE)), **wall)
    floor = b.material(b.translate((0, -1.0, 0), b.primitive(ft.PLANE)), colour=(0.5, 0.6, 0.7))
    ball = b.material(b.transform([("scale", 0.6), ("translate", (0.4, -0.2, 0.3))], b.primitive(ft.SPHERE)), colour=(0.9, 0.3, 0.2),
                      reflectance=0.4 if fancy else 0.0, shineyness=100.0 if fancy else 10.0, roughness=0.0)
    b.set_objects(b.group([back, front, floor, ball]))
    b.add_positional((0.5, 2.5, -0.5), (1.0, 0.02, 0.01), (1.0, 0.95, 0.9))
    b.commit()


MIRROR_CAMERA = ((-1.2, 0.6, -2.2), (0.6, -0.2, 3.0), (0, 1, 0), 50.0)
DEPTHS = (8, 9, 12, 15, 16)


def mirror_rays(n=2000, seed=4):
    rng = np.random.default_rng(seed)
    o = rng.uniform((-1.5, -0.5, -2.5), (1.5, 1.5, 2.5), size=(n, 3))
    d = rng.normal(size=(n, 3)) * (0.35, 0.25, 1.0)
    return o, d

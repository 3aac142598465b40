"""Tools for tests/test_device_bvh.py: a catalogue of meshes at which parallel BVH builders go wrong, a numpy replay of the linear
builder's ordering rule (k_bvh_prepare, k_bvh_morton, Karras' radix tree of k_bvh_hierarchy, the height k_bvh_fit counts) and a
checker of the trees Context.mesh_trees() reads back from HBM.

Morton cell borders.  The replay's keys equal the device's as long as no box centre lies on the border of a Morton cell, where the
rounding of (c - lo) / w could move a key.  Every catalogue mesh keeps u * 1024 at least 1e-6 away from the whole numbers 1 .. 1023
(`key_margin`, asserted by the tests) with three exceptions, listed in `Entry.exact`, whose centre is the centre of the mesh bounds by
construction: every triangle of `identical` and `concentric`, and the one triangle of `spanning` that spans the mesh.  Their
coordinates are chosen so that c, c - lo, w and the quotient 0.5 are all exact in binary64: nothing is rounded, u * 1024 is 512.0."""
import math
from collections import namedtuple

import numpy as np

import functracer_amd as ft

INT32_MIN = -2 ** 31
LEAF_TRIS = 4                                     # kLeafTris of both builders
BLOB_SIZES = (7, 8, 9, 63, 64, 65, 255, 256, 257, 1025)

# tris: [n, 3, 3] vertices a, b, c; centre / radius: where the dense part is (cameras and rays aim there); exact: see the module docstring
Entry = namedtuple("Entry", "name tris centre radius exact")

# a triangle whose box is exactly centre +- h on every axis
_PATTERN = np.array([[-1.0, -1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0]])


def _boxed(centre, h):
    return np.asarray(centre, dtype=np.float64)[None, :] + h * _PATTERN


def blob(n, seed=11):
    """The Gaussian recipe of test_device_built_bvh_equals_host_built_bvh."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(n, 1, 3)) * 0.8
    return centres + rng.normal(size=(n, 3, 3)) * 0.08


def chain(d):
    """d identical triangles in Morton cell (0, 0, 0), one in each of the cells (2^k, 0, 0), (0, 2^k, 0), (0, 0, 2^k), k = 0 .. 9, and one
    in (1023, 1023, 1023): the radix tree peels one key bit per level and then halves the d equal keys by position."""
    cells = [(0, 0, 0)] * d
    for k in range(10):
        cells += [(2 ** k, 0, 0), (0, 2 ** k, 0), (0, 0, 2 ** k)]
    cells.append((1023, 1023, 1023))
    return np.stack([_boxed(np.array(c, dtype=np.float64) + 0.5, 0.25) for c in cells])


def _flat(seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((500, 3, 3))
    t[:, :, :2] = rng.uniform(-1.0, 1.0, size=(500, 1, 2)) + rng.normal(size=(500, 3, 2)) * 0.08
    t[:, :, 2] = 0.37
    # The triangles overlap, so a ray meets several of them at the same t up to the last bit, and which of them is "closest" is decided
    # by rounding that the oracle and the device do not share.  With one winding for all, every candidate has the same normal.
    flip = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])[:, 2] < 0.0
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


def _degenerate():
    b = blob(500, seed=12)
    out = []
    for j in range(100):
        out.extend(b[5 * j:5 * j + 5])
        p, q = b[5 * j, 0], b[5 * j, 1]
        out.append(np.stack([p, p, q]) if j % 2 == 0 else np.stack([p, q, p + 0.5 * (q - p)]))   # two equal vertices | three collinear
    return np.stack(out)


def _geometric():
    t = [_boxed(np.full(3, 16.0 ** -k), 0.1 * 16.0 ** -k) for k in range(32)]
    t += [_boxed(np.zeros(3), 0.1 * 16.0 ** -31)] * 64
    return np.stack(t)


def _two_clusters():
    rng = np.random.default_rng(13)
    far = np.full(3, 1e3 / math.sqrt(3.0))
    parts = [p + rng.normal(size=(400, 1, 3)) * 2e-3 + rng.normal(size=(400, 3, 3)) * 1e-3 for p in (np.zeros(3), far)]
    return np.concatenate(parts)


def _spanning():
    rng = np.random.default_rng(14)
    t = rng.uniform(-1.5, 1.5, size=(501, 1, 3)) + rng.normal(size=(501, 3, 3)) * 0.05
    t[250] = _boxed(np.zeros(3), 2.0)
    return t


def _entry(name, tris, centre=None, radius=None, exact=()):
    tris = np.ascontiguousarray(tris, dtype=np.float64)
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    centre = 0.5 * (lo + hi) if centre is None else np.asarray(centre, dtype=np.float64)
    radius = 0.5 * float(np.linalg.norm(hi - lo)) if radius is None else float(radius)
    return Entry(name, tris, centre, radius, frozenset(exact))


def make_catalogue():
    """name -> Entry, every mesh of at most 2079 triangles, built from fixed seeds."""
    out = {}
    for n in BLOB_SIZES:
        out[f"blob({n})"] = _entry(f"blob({n})", blob(n))
    flat = _flat(15)
    entries = [
        _entry("identical", np.stack([_boxed(np.zeros(3), 0.5)] * 300), exact=range(300)),
        _entry("concentric", np.stack([_boxed(np.zeros(3), 0.25 * 1.01 ** i) for i in range(200)]), exact=range(200)),
        _entry("flat", flat),
        _entry("flat_x", flat[:, :, [2, 0, 1]]),                            # the same triangles rotated into the plane x = 0.37
        _entry("two_clusters", _two_clusters(), centre=np.zeros(3), radius=0.02),
        _entry("spanning", _spanning(), exact=[250]),
        _entry("degenerate", _degenerate()),
        _entry("chain(256)", chain(256), centre=np.full(3, 0.5), radius=1.5),
        _entry("chain(1024)", chain(1024), centre=np.full(3, 0.5), radius=1.5),
        _entry("chain(2048)", chain(2048), centre=np.full(3, 0.5), radius=1.5),
        _entry("geometric", _geometric(), centre=np.full(3, 0.5), radius=1.2),
    ]
    for e in entries:
        out[e.name] = e
    for e in out.values():
        e.tris.setflags(write=False)
    return out


_CACHE = {}


def catalogue():
    """make_catalogue(), built once per process and never modified."""
    if not _CACHE:
        _CACHE.update(make_catalogue())
    return _CACHE


# ------------------------------------------------------------------------------------------------------------ scenes, cameras, rays
def build_scene(b, tris):
    """One `bspMesh 0` of `tris` under two lights, committed in builder `b` (a Context or the oracle)."""
    b.clear()
    b.set_objects(b.group([b.material(b.bsp_mesh(0, np.asarray(tris).reshape(-1, 9)), colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    b.add_directional((1, -2, 1), (1, 1, 1))
    b.add_positional((2, 3, -2), (1, 0.1, 0.01), (0.5, 0.5, 1.0))
    b.commit()


MULTI_PARTS = [                                                      # (mesh, bspMesh depth, transforms: first listed applied first)
    ("blob(8)", 0, [("rotate", (0, 1, 0), 0.7), ("scale", (0.5, 0.5, 0.5)), ("translate", (-2.5, 0.5, 0.0))]),
    ("blob(257)", 0, [("rotate", (1, 0, 0), -0.4), ("scale", (0.8, 1.1, 0.9)), ("translate", (2.5, -0.3, 0.5))]),
    ("blob(1025)", 0, [("rotate", (0, 0, 1), 1.1), ("scale", (1.2, 1.2, 1.2)), ("translate", (0.0, 0.2, 4.0))]),
    ("blob(7)", 0, [("translate", (0.0, 2.5, 0.0))]),
    ("blob(63)", 3, [("scale", (0.7, 0.7, 0.7)), ("translate", (0.0, -2.5, 1.0))]),
]
MULTI_VIEW = (np.array([0.0, 0.0, 1.5]), 6.0)


def build_multi(b, extra=None):
    """Several meshes in one scene, each under its own rotate, scale and translate, around a sphere; `extra`: one more `bspMesh 0`."""
    cat = catalogue()
    b.clear()
    nodes = []
    for name, depth, ops in MULTI_PARTS:
        nodes.append(b.transform(ops, b.material(b.bsp_mesh(depth, cat[name].tris.reshape(-1, 9)), colour=(0.4, 0.8, 0.5), shineyness=2.0)))
        if name == "blob(257)":
            nodes.append(b.material(b.primitive(ft.SPHERE), colour=(0.8, 0.2, 0.2)))
    if extra is not None:
        nodes.append(b.transform([("scale", (1.0 / 256.0,) * 3), ("translate", (-1.0, -1.0, 6.0))], b.bsp_mesh(0, np.asarray(extra).reshape(-1, 9))))
    b.set_objects(b.group(nodes))
    b.add_directional((1, -2, 1), (1, 1, 1))
    b.commit()


def camera(centre, radius):
    """A camera far enough out that the corners of the frame look past the sphere (centre, radius)."""
    o = np.asarray(centre) + radius * np.array([0.9, 1.3, -3.6])
    return ft.make_camera(tuple(o), tuple(centre), (0, 1, 0), math.radians(50.0), 1.0)


def rays_for(view, tris=None, n=20000, seed=5):
    """About n rays (origins, directions, lengths for `blocked`) for the view (centre, radius): random ones aimed at the dense part,
    axis-parallel ones through triangle centres (along a chain's axes, inside the plane of a flat mesh) and rays that start inside the
    mesh bounds."""
    centre, radius = np.asarray(view[0], dtype=np.float64), float(view[1])
    rng = np.random.default_rng(seed)
    n_rand, n_axis, n_in = (n * 3) // 5, n // 5, n // 5
    o, d = [], []
    ro, rd = _random_rays(n_rand, seed + 1, radius * 1.2, centre, radius * 0.35)
    o.append(ro), d.append(rd)
    if tris is not None:
        # not at a zero-area triangle: whether a ray through its edge-on sliver hits it is decided by the last bit of a determinant
        area = np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1)
        cents = tris[area > 1e-9 * area.max()].mean(axis=1)
    else:
        cents = centre[None, :] + rng.normal(size=(64, 3)) * radius * 0.3
    pick = cents[rng.integers(0, cents.shape[0], size=n_axis)]
    axis = rng.integers(0, 3, size=n_axis)
    sign = rng.choice([-1.0, 1.0], size=n_axis)
    ad = np.zeros((n_axis, 3))
    ad[np.arange(n_axis), axis] = sign * rng.uniform(0.5, 2.0, size=n_axis)
    o.append(pick - ad * (3.0 * radius)), d.append(ad)
    lo, hi = (tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)) if tris is not None else (centre - radius, centre + radius)
    inside = np.concatenate([rng.uniform(lo, hi, size=(n_in // 2, 3)), cents[rng.integers(0, cents.shape[0], size=n_in - n_in // 2)] + rng.normal(size=(n_in - n_in // 2, 3)) * radius * 0.05])
    o.append(inside), d.append(rng.normal(size=(n_in, 3)) * rng.uniform(0.2, 3.0, size=(n_in, 1)))
    o, d = np.concatenate(o), np.concatenate(d)
    md = np.abs(rng.normal(size=o.shape[0])) * radius * 2.0
    return o, d, md


def _random_rays(n, seed, origin_scale, toward, spread):
    from . import helpers as H
    o, d = H.random_rays(n, seed=seed, origin_scale=origin_scale, toward=(0, 0, 0), spread=spread)
    return o + np.asarray(toward)[None, :], d


# ------------------------------------------------------------------------------------------------------------ the linear builder's order
def _records(tris_abc):
    """The triangle records the flattener stores (v0, e1 = b - a, e2 = c - a) and the vertices the hit test sees (v0, v0 + e1, v0 + e2)."""
    t = np.asarray(tris_abc, dtype=np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return np.stack([v0, v0 + e1, v0 + e2], axis=1)


def _spread3(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton_u(tris_abc):
    """Per triangle and axis, the box centre inside the mesh bounds scaled to 0 .. 1024 (k_bvh_morton before the clamp)."""
    v = _records(tris_abc)
    lo, hi = v.min(axis=1), v.max(axis=1)
    mlo, mhi = lo.min(axis=0), hi.max(axis=0)
    c = 0.5 * (lo + hi)
    w = mhi - mlo
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(w > 0.0, (c - mlo) / w, 0.0)
    return u * 1024.0


def morton_keys(tris_abc):
    q = np.minimum(np.maximum(morton_u(tris_abc), 0.0), 1023.0).astype(np.uint32)
    return (_spread3(q[:, 0]) << np.uint32(2)) | (_spread3(q[:, 1]) << np.uint32(1)) | _spread3(q[:, 2])


def key_margin(tris_abc, exact=()):
    """The smallest distance of any u * 1024 from a border between two Morton cells (the whole numbers 1 .. 1023), over the triangles not in
    `exact`; those must sit at 512.0 exactly."""
    u = morton_u(tris_abc)
    keep = np.ones(u.shape[0], dtype=bool)
    if exact:
        idx = np.fromiter(exact, dtype=np.int64)
        keep[idx] = False
        w = np.ptp(_records(tris_abc).reshape(-1, 3), axis=0)
        assert (u[idx][:, w > 0.0] == 512.0).all(), "an `exact` triangle is not at the centre of the mesh bounds"
    r = np.clip(np.rint(u[keep]), 1.0, 1023.0)
    return float(np.abs(u[keep] - r).min()) if keep.any() else math.inf


def replay_linear(tris_abc):
    """The linear builder's order and tree: (keys, order, height, walked_height).  order = stable argsort of the 30-bit keys (sorted position
    -> triangle); height as k_bvh_fit counts it (a triangle 0, a node 1 + its taller child); walked_height the same over the tree
    k_bvh_emit writes, where a node of at most four triangles stands as a leaf (0)."""
    keys = morton_keys(tris_abc)
    order = np.argsort(keys, kind="stable")
    sk = [int(k) for k in keys[order]]
    n = len(sk)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        a, b = sk[i], sk[j]
        if a != b:
            return 32 - (a ^ b).bit_length()
        return 32 + 32 - (i ^ j).bit_length()

    left, right, size = [0] * (n - 1), [0] * (n - 1), [0] * (n - 1)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, (l + 1) // 2
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t == 1:
                break
            t = (t + 1) // 2
        gamma = i + s * d + (-1 if d < 0 else 0)
        lo, hi = min(i, j), max(i, j)
        left[i] = ~gamma if lo == gamma else gamma
        right[i] = ~(gamma + 1) if hi == gamma + 1 else gamma + 1
        size[i] = hi - lo + 1
    fit, walked = [None] * (n - 1), [None] * (n - 1)
    stack = [0]
    while stack:                                                    # post-order without recursion
        i = stack[-1]
        kids = [c for c in (left[i], right[i]) if c >= 0]
        todo = [c for c in kids if fit[c] is None]
        if todo:
            stack.extend(todo)
            continue
        stack.pop()
        fit[i] = 1 + max([fit[c] for c in kids], default=0)
        walked[i] = 0 if size[i] <= LEAF_TRIS else 1 + max([walked[c] for c in kids], default=0)
    return keys, order, fit[0], walked[0]


# ------------------------------------------------------------------------------------------------------------ the structure checker
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _wide_children(T):
    return np.ascontiguousarray(T["wide"]).view(np.int32).reshape(-1, 56)[:, 48:52]


def check_trees(T, device_bvh_height=None, replays=None):
    """Walk what Context.mesh_trees() returned and assert, for every top-level-Leaf mesh with a BVH, what tests/test_device_bvh.py lists:
    every triangle once, boxes that hold what is below them, a 4-wide tree over the same leaves, coarse boxes over every triangle, depths
    within the walkers' stacks, jobs that do not overlap and (replays: mesh index -> replay_linear's result) the linear builder's order.
    Returns one report per checked mesh."""
    nodes, leaves, tris, tri_orig, tri_src, wide, coarse, meshes = (T[k] for k in ("nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes"))
    assert tri_orig.shape[0] == tris.shape[0] == tri_src.shape[0], "one tri_orig and one tri_src entry per triangle record"
    wchild = _wide_children(T)
    verts = np.stack([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]], axis=1)   # as the hit test sees them
    tlo, thi = verts.min(axis=1), verts.max(axis=1)
    jobs = {j["mesh"]: j for j in T["jobs"]}
    assert len(jobs) == len(T["jobs"]), "two jobs for one mesh"
    _check_jobs_disjoint(T)
    if T["jobs"]:
        assert device_bvh_height is None or 0 < device_bvh_height <= 40, f"device_bvh_height {device_bvh_height}"
    reports = []
    for m, (root, bvh_root, n_src, wide_root, coarse_first, coarse_count) in enumerate(meshes.tolist()):
        if root >= 0 or bvh_root == INT32_MIN:
            continue
        what = f"mesh {m}"
        first_global, n = (int(x) for x in leaves[~root])
        job = jobs.get(m)
        if job is not None:
            assert (job["first_global"], job["n"]) == (first_global, n) and bvh_root == job["node_base"] and wide_root == job["wide_base"], f"{what}: job and mesh tables disagree"
            assert (coarse_first, coarse_count) == (job["coarse_first"], job["coarse_count"]), f"{what}: coarse range"
        extent = float(np.abs(verts[first_global:first_global + n]).max())
        pad = 1e-7 * extent + 1e-300                                 # the builders' own inflation
        half = 0.5 * pad

        def need_of_leaf(ref):
            f, c = (int(x) for x in leaves[~ref])
            assert c >= 1, f"{what}: leaf {~ref} is empty"
            assert c <= LEAF_TRIS, f"{what}: leaf {~ref} holds {c} triangles"
            assert f + c <= tris.shape[0], f"{what}: leaf {~ref} runs past the triangle array"
            if job is not None:
                assert job["tri_base"] <= f and f + c <= job["tri_base"] + n, f"{what}: leaf {~ref} outside the job's triangle range"
                assert job["leaf_base"] <= ~ref < job["leaf_base"] + 2 * n - 1, f"{what}: leaf {~ref} outside the job's leaf range"
            return tlo[f:f + c].min(axis=0), thi[f:f + c].max(axis=0)

        # ---- the binary tree: post-order, the bounds every subtree needs, its height in node levels
        assert bvh_root >= 0, f"{what}: bvh_root {bvh_root}"
        need, height, leaf_refs, seen = {}, {}, [], set()
        stack = [bvh_root]
        while stack:
            r = stack[-1]
            if r < 0:
                stack.pop()
                if r not in need:
                    need[r] = need_of_leaf(r)
                    height[r] = 0
                    leaf_refs.append(r)
                else:
                    raise AssertionError(f"{what}: leaf {~r} reached twice")
                continue
            if r not in seen:
                assert r < nodes.shape[0], f"{what}: node {r} outside the node array"
                if job is not None:
                    assert job["node_base"] <= r < job["node_base"] + n - 1, f"{what}: node {r} outside the job's node range"
                assert len(seen) < 2 * n, f"{what}: the tree does not end"
                seen.add(r)
                l, rr = int(nodes["left"][r]), int(nodes["right"][r])
                assert l not in seen and rr not in seen and l != rr, f"{what}: node {r} points back into the tree"
                stack.extend([rr, l])
                continue
            stack.pop()
            l, rr = int(nodes["left"][r]), int(nodes["right"][r])
            lo, hi = np.minimum(need[l][0], need[rr][0]), np.maximum(need[l][1], need[rr][1])
            need[r] = (lo, hi)
            height[r] = 1 + max(height[l], height[rr])
            bmin, bmax = nodes["bmin"][r], nodes["bmax"][r]
            assert (bmin <= lo - half).all() and (bmax >= hi + half).all(), f"{what}: the box of node {r} does not hold what is below it (by {np.maximum(bmin - lo, hi - bmax).max():.3e}, pad {pad:.3e})"
            assert int(nodes["axis"][r]) in (0, 1, 2), f"{what}: node {r} axis {nodes['axis'][r]}"
            for c in (l, rr):                                       # a child's box lies inside its parent's
                if c >= 0:
                    assert (nodes["bmin"][c] >= bmin).all() and (nodes["bmax"][c] <= bmax).all(), f"{what}: the box of node {c} sticks out of its parent's ({r})"
        rlo, rhi = need[bvh_root]
        assert (nodes["bmin"][bvh_root] >= rlo - 2.0 * pad).all() and (nodes["bmax"][bvh_root] <= rhi + 2.0 * pad).all(), f"{what}: the root box is wider than the mesh and its pad"

        # ---- every triangle once
        ranges = sorted((int(leaves[~r][0]), int(leaves[~r][1])) for r in leaf_refs)
        for (f0, c0), (f1, _) in zip(ranges, ranges[1:]):
            assert f0 + c0 <= f1, f"{what}: leaf ranges overlap at {f1}"
        ks = np.concatenate([np.arange(f, f + c) for f, c in ranges])
        assert ks.shape[0] == n, f"{what}: the leaves hold {ks.shape[0]} triangles of {n}"
        assert not np.any((ks >= first_global) & (ks < first_global + n)), f"{what}: a BVH leaf reads the reference-order list"
        assert np.array_equal(np.sort(tri_orig[ks]), np.arange(first_global, first_global + n, dtype=np.uint32)), f"{what}: tri_orig is not a permutation of the mesh's triangles"
        assert np.array_equal(_bits(tris[ks]), _bits(tris[tri_orig[ks]])), f"{what}: a sorted triangle record is not its tri_orig's record"
        assert np.array_equal(tri_src[ks], tri_src[tri_orig[ks]]), f"{what}: tri_src of a sorted record"

        # ---- the 4-wide tree, walked on its own
        assert wide_root >= 0, f"{what}: no 4-wide tree"
        wneed, wdepth, wleaves = {}, {}, []

        def wide_walk(w, level):
            assert 0 <= w < wide.shape[0] and w not in wneed, f"{what}: wide node {w}"
            assert level <= 64, f"{what}: the 4-wide tree does not end"
            if job is not None:
                assert job["wide_base"] <= w < job["wide_base"] + n - 1, f"{what}: wide node {w} outside the job's range"
            lo, hi, depth = np.full(3, np.inf), np.full(3, -np.inf), 1
            wneed[w] = None
            for s in range(4):
                c, box = int(wchild[w, s]), wide[w, 6 * s:6 * s + 6]
                if c == INT32_MIN:
                    assert np.isnan(box).all(), f"{what}: empty slot {s} of wide node {w} has a box"
                    continue
                if c < 0:
                    clo, chi = need_of_leaf(c)
                    wleaves.append(c)
                else:
                    clo, chi, d = wide_walk(c, level + 1)
                    depth = max(depth, 1 + d)
                assert (box[:3] <= clo - half).all() and (box[3:] >= chi + half).all(), f"{what}: slot {s} of wide node {w} does not hold what is below it"
                lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
            assert np.isfinite(lo).all(), f"{what}: wide node {w} is empty"
            wneed[w] = (lo, hi)
            return lo, hi, depth

        wide_depth = wide_walk(wide_root, 1)[2]
        assert sorted(wleaves) == sorted(leaf_refs), f"{what}: the 4-wide tree reaches other leaves than the binary tree"
        assert 3 * wide_depth <= 64, f"{what}: 4-wide depth {wide_depth} needs more than the packet walk's 64 stack entries"
        if job is not None:
            _check_wide_bitwise(T, job, wchild, tlo, thi, pad, what)

        # ---- coarse boxes
        assert coarse_count >= 1 and coarse_first + coarse_count <= coarse.shape[0], f"{what}: coarse range"
        cb = coarse[coarse_first:coarse_first + coarse_count].astype(np.float64)
        a, b = tlo[first_global:first_global + n], thi[first_global:first_global + n]
        held = ((cb[None, :, :3] <= a[:, None, :]) & (cb[None, :, 3:] >= b[:, None, :])).all(axis=2).any(axis=1)
        assert held.all(), f"{what}: no coarse box holds triangles {np.nonzero(~held)[0][:5]}"
        if job is not None:                                          # one level of the tree, the last box repeated up to the count
            frontier = [bvh_root]
            while True:
                nxt = []
                for c in frontier:
                    nxt.extend([c] if c < 0 else [int(nodes["left"][c]), int(nodes["right"][c])])
                if len(nxt) > 64 or all(c < 0 for c in frontier):
                    break
                frontier = nxt
            for k in range(coarse_count):
                flo, fhi = need[frontier[min(k, len(frontier) - 1)]]
                assert (cb[k, :3] <= flo).all() and (cb[k, 3:] >= fhi).all(), f"{what}: coarse box {k} is not the box of its node of the level"
                if k >= len(frontier):
                    assert np.array_equal(_bits(coarse[coarse_first + k]), _bits(coarse[coarse_first + len(frontier) - 1])), f"{what}: coarse box {k} does not repeat the last one"

        # ---- depth
        h = height[bvh_root]
        assert h <= 40, f"{what}: height {h}"
        assert h + 1 <= T["stack_capacity"], f"{what}: height {h} does not fit the per-lane stacks of {T['stack_capacity']}"
        if job is not None and device_bvh_height is not None:
            assert h <= device_bvh_height, f"{what}: walked height {h} above the reported {device_bvh_height}"
            assert device_bvh_height + 1 <= T["stack_capacity"], f"reported height {device_bvh_height}, stacks of {T['stack_capacity']}"

        # ---- the linear builder's order
        if replays is not None and m in replays:
            assert job is not None, f"{what}: not device-built"
            _, order, fit_height, walked_height = replays[m]
            got = tri_orig[job["tri_base"]:job["tri_base"] + n].astype(np.int64) - first_global
            assert np.array_equal(got, order), f"{what}: tri_orig is not the stable Morton order (first difference at sorted position {np.nonzero(got != order)[0][:1]})"
            assert h == walked_height, f"{what}: walked height {h}, replayed {walked_height}"
            if device_bvh_height is not None and len(T["jobs"]) == 1:
                assert device_bvh_height == fit_height, f"{what}: reported height {device_bvh_height}, replayed {fit_height}"
        reports.append({"mesh": m, "device_built": job is not None, "height": h, "wide_depth": wide_depth, "n": n, "first_global": first_global,
                        "bvh_root": bvh_root, "need": need, "leaf_refs": leaf_refs})
    return reports


def _check_wide_bitwise(T, job, wchild, tlo, thi, pad, what):
    """Device-built: wide node i is binary node i two levels at a time, its slot boxes bitwise the padded boxes of the grandchildren."""
    nodes, leaves, wide = T["nodes"], T["bsp_leaves"], T["wide"]
    n = job["n"]

    def padded(ref):
        if ref >= 0:
            return np.concatenate([nodes["bmin"][ref], nodes["bmax"][ref]])
        k = ~ref - job["leaf_base"]
        if k < n - 1:                                               # a node of the build standing as a leaf: its record was written all the same
            return np.concatenate([nodes["bmin"][job["node_base"] + k], nodes["bmax"][job["node_base"] + k]])
        f, c = (int(x) for x in leaves[~ref])
        return np.concatenate([tlo[f:f + c].min(axis=0) - pad, thi[f:f + c].max(axis=0) + pad])

    stack = [job["node_base"]]
    while stack:
        r = stack.pop()
        w = job["wide_base"] + (r - job["node_base"])
        want_child, want_box = [INT32_MIN] * 4, [None] * 4
        for hside, c in enumerate((int(nodes["left"][r]), int(nodes["right"][r]))):
            if c < 0:
                want_child[2 * hside], want_box[2 * hside] = c, padded(c)
                continue
            for k, g in enumerate((int(nodes["left"][c]), int(nodes["right"][c]))):
                want_child[2 * hside + k] = g if g < 0 else job["wide_base"] + (g - job["node_base"])
                want_box[2 * hside + k] = padded(g)
                if g >= 0:
                    stack.append(g)
        assert wchild[w].tolist() == want_child, f"{what}: wide node {w} children {wchild[w].tolist()}, binary node {r} gives {want_child}"
        for s in range(4):
            if want_box[s] is not None:
                assert np.array_equal(_bits(wide[w, 6 * s:6 * s + 6]), _bits(want_box[s])), f"{what}: slot {s} of wide node {w} is not the padded box of its binary grandchild"


def _check_jobs_disjoint(T):
    spans = {"nodes": [], "bsp_leaves": [], "tris": [], "wide": [], "coarse_boxes": []}
    for j in T["jobs"]:
        n = j["n"]
        assert n >= 8, f"job of {n} triangles"
        spans["nodes"].append((j["node_base"], n - 1))
        spans["bsp_leaves"].append((j["leaf_base"], 2 * n - 1))
        spans["tris"].append((j["tri_base"], n))
        spans["tris"].append((j["first_global"], n))                # the reference-order list the job reads
        spans["wide"].append((j["wide_base"], n - 1))
        spans["coarse_boxes"].append((j["coarse_first"], j["coarse_count"]))
    for name, s in spans.items():
        s.sort()
        for (a, c), (b, _) in zip(s, s[1:]):
            assert a + c <= b, f"two jobs overlap in {name} at {b}"
        if s:
            assert s[-1][0] + s[-1][1] <= T[name].shape[0], f"a job runs past the end of {name}"

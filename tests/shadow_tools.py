"""Scenes, CPU proofs and structure checks for tests/test_light_space_hard.py: the hard-mesh catalogue of tests/bvh_tools.py as shadow
CASTER over a receiver, under directional lights, so that the light-space tree and grid of the mesh (ft_scene.cpp, build_light_space;
ft_kernels.hip, mesh_shadow_packet / mesh_shadow_grid) answer shadow queries from the mesh's own surface and from points far outside its
(u, v) extent.

A case is a function of a builder, so the oracle, a host-only context and the device build the same scene.  Its geometry follows from a few
numbers: the receiver is a scaled SQUARE whose normal is the bisector of the directions towards the lights, `recv[0]` mesh radii behind the
mesh; the eye stands `cam.dist` radii from a point between receiver and mesh, `cam.el` degrees above the receiver's plane.  A low eye makes
the pixel footprints on the receiver long, so some waves cover many grid cells (the tree route) and others one (the grid route).

Waves.  k_primary takes batches of B consecutive entries of the pixel list, B = batch_lanes_for(n, lane_fold, n_simd): the largest power
of two <= 64 with B * n_simd <= n.  A full frame whose sides are multiples of 8 is listed in 8x8 blocks, Z order inside (ft_frame.cpp,
list_pixels), so a wave is an aligned square of B pixels: the whole block from 65536 pixels up on the 1024 SIMDs of an MI355X, and a 2x2
square at the 96 x 72 pixels of these frames.  At 4 samples the numbering is grouped (slot_at): a wave holds a 4x4 square under four
offsets.  route_counts classifies all three at jitter (0, 0): `blocks` (8x8), `quads` (2x2) and `sixteens` (4x4); the conditions are
asserted for the first two.

The eye, the receiver's distance and, for the sparse blobs, the triangle whose shadow the eye looks at (`aim`) were found by a search over
a few hundred candidates per case on the oracle and the host builder alone, for the conditions at the end of this file."""
import functools
import math
from collections import namedtuple

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import bvh_tools as B
from . import walk_tools as W
from .test_light_space_grid import cell, grid_of
from .test_light_space_shadows import NONE, light_space, pair_root

WAVE_STACK = 64                                   # entries of the WaveStack of ls_tree_walk
GRID_WAVE_CELLS = 4                               # kLsGridWaveCells
LS_MAX_TRIS = 1 << 20                             # kLsMaxTris
BINNED_LEVELS = 16                                # LsBuilder::build: `level < 16`
LEAF_TRIS = 4                                     # LsBuilder::kLeafTris
MARGIN = 1e-3                                     # of a cell: how far a wave's rectangle is widened / narrowed before it is classified
SLIGHT_OFFSET = 1e-4                              # Shading.fs:109-117: the shadow ray starts at p + 1e-4 n
MESH_COLOUR, RECEIVER_COLOUR = (0.8, 0.7, 0.6), (0.5, 0.5, 0.5)
MIRROR = [("scale", (-1.0, 1.0, 1.0))]
TILES = [(0, 0, 40, 24), (24, 16, 32, 32), (72, 48, 40, 40)]      # the last one hangs over the frame's edge
SELF_SHADOWING = ("degenerate", "concentric", "spanning", "two_clusters", "blob(1025)", "chain(256)")
TREE_ONLY = ("identical", "two_clusters", "chain(256)", "chain(2048)")

Cam = namedtuple("Cam", "az el dist fov tau")     # degrees, degrees, mesh radii, degrees, 0 = look at the receiver .. 1 = at the mesh
# parts: [(catalogue name, transform or None, "lit" | "unlit" | "same": the node before it again)]; lights: ("dir", v) | ("point", p) |
# ("soft", v, samples, scatter); recv: (distance behind the mesh, side), in mesh radii; aim: None or (part, triangle, light): the eye looks
# at that triangle's shadow on the receiver
Case = namedtuple("Case", "name parts lights cam recv w h tiles aim")

GENERAL, HAIR = (1.0, -2.0, 1.0), (1e-4, -1.0, 3e-5)
DIAGONAL = (-1.0, -1.0, -1.0)                     # along the diagonal `geometric` and `chain` are strung on, towards the origin


def _case(name, mesh, lights, cam, recv=(1.5, 16.0), ops=None, w=96, h=72, tiles=None, aim=None):
    return Case(name, [(mesh, ops, "lit")], [("dir", v) for v in lights], Cam(*cam), recv, w, h, tiles, aim)


def deep(n=4096, ratio=2.0 ** -0.2):
    """A mesh built for depth: n triangles whose centres and sizes are ratio^k along the diagonal.  Over 16 bins of the centroid extent the
    cheapest cut is the one before bin 1, whatever the light: area x count of the crowd near the origin shrinks by 256 while the few large
    triangles cost their count.  So each of the 16 binned levels peels the top fifteen sixteenths of the extent, and medians halve the
    rest: 16 + ceil(log2(rest / 4)) binary levels."""
    return np.stack([B._boxed(np.full(3, ratio ** k), 0.1 * ratio ** k) for k in range(n)])


@functools.lru_cache(maxsize=None)
def mesh_tris(name):
    if name == "deep(4096)":
        t = deep()
        t.setflags(write=False)
        return t
    return B.catalogue()[name].tris


def mesh_ball(name):
    """(centre, radius) of the dense part of a mesh."""
    if name == "deep(4096)":
        return np.full(3, 0.5), 1.0
    e = B.catalogue()[name]
    return e.centre, e.radius


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def dir_lights(case):
    """[(index among the scene's lights, direction the light travels)] of the directional lights."""
    return [(k, np.asarray(l[1], dtype=np.float64)) for k, l in enumerate(case.lights) if l[0] == "dir"]


def geometry(case):
    """The receiver's transform and the view of a case."""
    balls = []
    for mesh, ops, _ in case.parts:
        m, t = W.matrix(ops)
        c, r = mesh_ball(mesh)
        balls.append((m @ c + t, r * float(np.linalg.svd(m, compute_uv=False).max())))
    cw = np.mean([c for c, _ in balls], axis=0)
    rw = max(float(np.linalg.norm(c - cw)) + r for c, r in balls)
    n = -_unit(sum(_unit(l[1]) for l in case.lights if l[0] != "point"))           # towards the lights
    p = cw - case.recv[0] * rw * n
    side = case.recv[1] * rw
    ops = [("scale", (side, 1.0, side)), ("translate", (-0.5 * side, 0.0, -0.5 * side))]   # SQUARE: [0, 1]^2 of the plane y = 0
    axis, cosine = np.cross((0.0, 1.0, 0.0), n), float(n[1])
    if np.linalg.norm(axis) > 1e-12:
        ops.append(("rotate", tuple(axis), math.atan2(float(np.linalg.norm(axis)), cosine)))
    elif cosine < 0.0:
        ops.append(("rotate", (1.0, 0.0, 0.0), math.pi))
    ops.append(("translate", tuple(p)))
    a = int(np.argmin(np.abs(n)))
    s1 = _unit(np.cross(n, np.eye(3)[a]))
    s2 = np.cross(n, s1)
    az, el = math.radians(case.cam.az), math.radians(case.cam.el)
    target = p + case.cam.tau * (cw - p)
    if case.aim is not None:                                        # at the shadow of one triangle's centroid under one light, on the receiver
        part, tri, light = case.aim
        m, t = W.matrix(case.parts[part][1])
        q, v = m @ mesh_tris(case.parts[part][0])[tri].mean(axis=0) + t, np.asarray(case.lights[light][1], dtype=np.float64)
        target = q + v * (float((p - q) @ n) / float(v @ n))
    eye = target + case.cam.dist * rw * (math.cos(el) * (math.cos(az) * s1 + math.sin(az) * s2) + math.sin(el) * n)
    return ops, W.View(case.name, eye, target, case.cam.fov, case.w, case.h, case.tiles, None)


def build(b, case):
    """The case's scene in builder `b`: the casters first (leaf k is part k), the receiver last."""
    recv_ops, _ = geometry(case)
    b.clear()
    items, node = [], None
    for mesh, ops, kind in case.parts:
        if kind != "same":
            node = b.bsp_mesh(0, mesh_tris(mesh).reshape(-1, 9))
        item = b.material(b.transform(list(ops), node) if ops else node, colour=MESH_COLOUR)
        items.append(b.ignore_light(item) if kind == "unlit" else item)
    items.append(b.material(b.transform(recv_ops, b.primitive(ft.SQUARE)), colour=RECEIVER_COLOUR))
    b.set_objects(b.group(items))
    for l in case.lights:
        if l[0] == "dir":
            b.add_directional(l[1], (1, 1, 1))
        elif l[0] == "point":
            b.add_positional(l[1], (1.0, 0.0, 0.02), (0.5, 0.5, 1.0))
        else:
            b.add_soft_directional(l[1], l[2], l[3], (0.6, 0.6, 0.6))
    b.commit()


def view_of(case):
    return geometry(case)[1]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _cases():
    xf, xfm = list(W.XF), list(W.XF) + MIRROR
    out = [
        # name, mesh, lights, (az, el, dist, fov, tau), recv: found by a search over these numbers on the oracle alone, for the conditions below
        _case("blob(7)", "blob(7)", [GENERAL, (0, -1, 0)], (30, 8, 0.1, 25, 0.0), aim=(0, 0, 1)),
        _case("blob(8)", "blob(8)", [GENERAL, HAIR], (300, 8, 0.1, 25, 0.0), aim=(0, 0, 0)),
        _case("blob(9)", "blob(9)", [(0, 0, 1), HAIR], (210, 8, 0.1, 25, 0.0), aim=(0, 0, 0)),
        _case("blob(65)", "blob(65)", [GENERAL, (1, 0, 0)], (30, 8, 1.2, 25, 0.0)),
        _case("blob(1025)", "blob(1025)", [GENERAL, (0, -1, 0)], (30, 15, 2.0, 45, 0.4)),
        _case("identical", "identical", [GENERAL, (0, 0, 1)], (30, 25, 5.0, 40, 0.3), recv=(2.0, 16.0)),
        _case("concentric", "concentric", [(0, 0, 1), DIAGONAL], (30, 15, 0.4, 45, 0.5)),
        _case("concentric-general", "concentric", [GENERAL, HAIR], (30, 15, 3.5, 45, 0.4)),
        _case("flat-in-plane", "flat", [GENERAL, (1, 0, 0)], (30, 8, 0.7, 25, 0.0)),
        _case("flat-off-plane", "flat", [(0, 0, 1), (1, 0, 1e-3)], (30, 25, 5.0, 40, 0.3), recv=(2.0, 16.0)),
        _case("flat_x-in-plane", "flat_x", [GENERAL, (0, -1, 0)], (30, 8, 0.7, 25, 0.0)),
        _case("flat_x-off-plane", "flat_x", [(1, 0, 0), (1e-3, -1, 0)], (30, 25, 5.0, 40, 0.3), recv=(2.0, 16.0)),
        _case("two_clusters", "two_clusters", [GENERAL, (0, -1, 0)], (30, 25, 3.5, 25, 0.4)),
        _case("spanning", "spanning", [GENERAL, HAIR], (30, 25, 5.0, 40, 0.3), recv=(2.0, 16.0)),
        _case("degenerate", "degenerate", [GENERAL, (0, 0, 1)], (30, 8, 1.2, 45, 0.4)),
        _case("chain(256)", "chain(256)", [DIAGONAL, GENERAL], (30, 25, 5.0, 40, 0.3), recv=(2.0, 16.0)),
        _case("geometric", "geometric", [DIAGONAL, HAIR], (30, 8, 1.2, 45, 0.0)),
        _case("blob(65)-xf", "blob(65)", [GENERAL, (0, -1, 0)], (210, 50, 1.5, 25, 0.5), ops=xf),
        _case("blob(65)-mirror", "blob(65)", [GENERAL, HAIR], (300, 50, 1.5, 25, 0.5), ops=xfm),
        _case("degenerate-xf", "degenerate", [GENERAL, HAIR], (30, 45, 2.0, 45, 0.4), ops=xf),
        _case("degenerate-mirror", "degenerate", [GENERAL, (1, 0, 0)], (30, 15, 2.0, 45, 0.4), ops=xfm),
        _case("concentric-xf", "concentric", [GENERAL, (0, 0, 1)], (30, 15, 2.0, 45, 0.8), ops=xf),
        _case("concentric-mirror", "concentric", [GENERAL, (0, -1, 0)], (30, 45, 1.2, 45, 0.8), ops=xfm),
        _case("spanning-tiles", "spanning", [GENERAL, (0, -1, 0)], (30, 45, 1.2, 25, 0.4), tiles=TILES),
        _case("two-lights-apart", "spanning", [(2, -1, 0), (-2, -1, 0)], (30, 15, 1.5, 45, 0.0), recv=(1.0, 16.0)),
    ]
    far = [("rotate", (0.0, 1.0, 0.0), 0.9), ("scale", (2.5, 3.0, 2.2)), ("translate", (0.5, 0.3, 2.5))]
    parts = [("blob(8)", [("translate", (-2.5, 0.0, 0.0))], "lit"), ("blob(7)", [("translate", (2.5, 0.5, 0.0))], "lit"),
             ("blob(65)", [("translate", (0.0, 0.0, -2.5))], "unlit"), ("blob(65)", far, "same")]
    lights = [("soft", (0.5, -2.0, 0.3), 3, 0.05), ("point", (0.0, 6.0, 0.0)), ("dir", GENERAL), ("dir", (-1.0, -2.0, 0.5))]
    out.append(Case("multi-leaf", parts, lights, Cam(300, 70, 0.4, 45, 0.5), (1.0, 16.0), 96, 72, None, None))
    return {c.name: c for c in out}


CASES = _cases()
SINGLE = [n for n, c in CASES.items() if len(c.parts) == 1]
MESHES = ("blob(7)", "blob(8)", "blob(9)", "blob(65)", "blob(1025)", "identical", "concentric", "flat", "flat_x", "two_clusters", "spanning",
          "degenerate", "chain(256)", "geometric")


# ---------------------------------------------------------------------------------------------------------------- the host builder
@functools.lru_cache(maxsize=None)
def structures(name):
    """What the host builder makes of the case: light_space() of a host-only context."""
    ctx = ft.Context(host_only=True)
    build(ctx, CASES[name])
    out = light_space(ctx)
    ctx.close()
    for a in out:
        a.setflags(write=False)
    return out


def mesh_structures(mesh, lights):
    """The same for a bare mesh under directional lights (no receiver)."""
    ctx = ft.Context(host_only=True)
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.material(ctx.bsp_mesh(0, mesh_tris(mesh).reshape(-1, 9)), colour=MESH_COLOUR)]))
    for v in lights:
        ctx.add_directional(v, (1, 1, 1))
    ctx.commit()
    out = light_space(ctx)
    ctx.close()
    return out


def pairs_of(name, part=0):
    """[(light index, pair record)] of the directional lights of one caster of a case; [] when the leaf has no pairs."""
    pairs, _, _, leaf_pairs = structures(name)
    base = int(leaf_pairs[part])
    if base == 0xFFFFFFFF:
        return []
    return [(l, pairs[base + l]) for l, _ in dir_lights(CASES[name])]


def cell_counts(rec, nodes):
    """[n_v, n_u] entries per cell of a pair's grid."""
    at, _, nu, nv = grid_of(rec)
    words = np.asarray(nodes).reshape(-1)
    return words[at:at + 4 * nu * nv].reshape(nv, nu, 4)[:, :, 2].astype(np.int64)


def worst_stack(rec, nodes):
    """The largest number of pending entries of ls_tree_walk's stack over the pair's tree if every child were entered: at a node the slots
    3, 2 and 1 are pushed (an empty slot's box is NaN: never entered, never counted) and slot 0 is taken directly; a leaf pops the next."""
    kids = np.asarray(nodes)[:, 20:24].view(np.int32)
    worst = 0
    todo = [(pair_root(rec), 0)]                  # (node, entries pending when it is taken)
    while todo:
        n, sp = todo.pop()
        ch = [int(c) for c in kids[n]]
        assert ch[0] != NONE, "the first slot of a node is never empty"
        pushed = [c for c in (ch[3], ch[2], ch[1]) if c != NONE]
        worst = max(worst, sp + len(pushed))
        for k, c in enumerate([ch[0]] + pushed[::-1]):           # popped in the order 1, 2, 3: each with the later ones still pending
            if c >= 0:
                todo.append((c, sp + len(pushed) - k))
    return worst


def stack_bound(n_tris=LS_MAX_TRIS):
    """What LsBuilder::build implies for n triangles: 16 binned levels that may each peel one triangle, then medians down to leaves of four,
    two binary levels per 4-wide node, three pushes per 4-wide node on the way down."""
    rest, medians = n_tris, 0
    while rest > LEAF_TRIS:
        rest, medians = (rest + 1) // 2, medians + 1
    levels = BINNED_LEVELS + medians
    return 3 * ((levels + 1) // 2), levels


# ---------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def reference(name):
    """closest() of the oracle on the case's pixel rays at jitter (0, 0) and, per directional light, blocked() from every hit point
    towards the light with an unbounded length; computed once and shared."""
    case = CASES[name]
    view = view_of(case)
    orc = O.Oracle()
    build(orc, case)
    o, d, xs, ys = W.pixel_rays(view)
    hit, t, p, n, col = orc.closest(o + SLIGHT_OFFSET * d, d)
    hit = hit.astype(bool)
    origin = p + SLIGHT_OFFSET * n
    blocked = {}
    for l, v in dir_lights(case):
        b = np.zeros(len(hit), dtype=bool)
        b[hit] = orc.blocked(origin[hit], np.broadcast_to(-v, origin[hit].shape).copy(), np.full(int(hit.sum()), 1e300)).astype(bool)
        blocked[l] = b
    orc.close()
    receiver = hit & (np.abs(col - np.array(RECEIVER_COLOUR)).max(axis=1) < 1e-9)
    out = {"view": view, "xs": xs, "ys": ys, "hit": hit, "receiver": receiver, "mesh": hit & ~receiver, "origin": origin, "blocked": blocked}
    for a in (xs, ys, hit, receiver, origin) + tuple(blocked.values()):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_frame(name, spp):
    case = CASES[name]
    view = view_of(case)
    orc = O.Oracle()
    build(orc, case)
    frame, _ = orc.render(W.camera(view), view.w, view.h, spp, jitter(spp), tiles=view.tiles)
    orc.close()
    frame.setflags(write=False)
    return frame


def jitter(spp):
    return np.zeros((1, 2)) if spp == 1 else ft.jitter_pattern(spp)


def shadow_counts(name):
    """Per directional light: receiver pixels shadowed, receiver pixels lit, mesh pixels shadowed, mesh pixels lit."""
    ref = reference(name)
    return {l: (int((ref["receiver"] & b).sum()), int((ref["receiver"] & ~b).sum()), int((ref["mesh"] & b).sum()), int((ref["mesh"] & ~b).sum()))
            for l, b in ref["blocked"].items()}


def shadow_masks(name):
    """Per directional light, the frame's receiver pixels in the mesh's shadow, as a [h, w] mask."""
    ref = reference(name)
    out = {}
    for l, b in ref["blocked"].items():
        m = np.zeros((ref["view"].h, ref["view"].w), dtype=bool)
        m[ref["ys"], ref["xs"]] = ref["receiver"] & b
        out[l] = m
    return out


# ---------------------------------------------------------------------------------------------------------------- which route a wave takes
def _cell(x, s, n):
    """test_light_space_grid.cell, which is exact; through floating point where that cannot differ: a float32 rounds fmaf's result by at
    most 6e-8 of its size, so a value 1e-4 away from every whole number, or far outside 0 .. n, lands in the same cell either way."""
    y = float(x) * float(s) + 0.5 * n
    if y < -1.0 or y > n + 1.0:
        return 0 if y < 0.0 else n - 1
    if abs(y - round(y)) > 1e-4 and n <= 1024:
        return min(max(math.floor(y), 0), n - 1)
    return cell(x, s, n)


def _span(x, s, n, by):
    """(first, last) cell of the interval [min x - by, max x + by] (by in cells; negative narrows, never past the interval's middle)."""
    lo, hi = float(x.min()), float(x.max())
    pad = by / s
    if pad < 0.0:
        pad = -min(-pad, 0.5 * (hi - lo))
    return _cell(lo - pad, s, n), _cell(hi + pad, s, n)


def route_counts(name, light, rec, nodes, part=0, cell_span=_span):
    """Classify the waves of a full 1-sample frame for one pair.  Per wave shape ("blocks": 8x8, "quads": 2x2; the module docstring):
    grid / tree: waves that surely take that route; full: surely-grid waves that surely visit a cell of more than 64 entries; outside:
    waves with a receiver lane whose unclamped cell index lies outside the grid."""
    case, ref = CASES[name], reference(name)
    assert case.tiles is None and case.w % 8 == 0 and case.h % 8 == 0
    at, s, nu, nv = grid_of(rec)
    assert nu > 0
    m, t = W.matrix(case.parts[part][1])
    model = (ref["origin"] - t) @ np.linalg.inv(m).T              # shade_lights traces from p + 1e-4 n; to_model takes it into the mesh's space
    rel = model - rec[9:12]
    u, v = rel @ rec[0:3], rel @ rec[3:6]
    send = ref["hit"]                                              # every material of these scenes is lit: every hit lane sends a shadow ray
    fu, fv = np.floor(u * s + 0.5 * nu), np.floor(v * s + 0.5 * nv)
    off = ref["receiver"] & ((np.minimum(u * s + 0.5 * nu, v * s + 0.5 * nv) < -MARGIN) | (u * s + 0.5 * nu > nu + MARGIN) | (v * s + 0.5 * nv > nv + MARGIN))
    assert np.isfinite(fu[send]).all() and np.isfinite(fv[send]).all()
    counts = cell_counts(rec, nodes)
    xs, ys = ref["xs"], ref["ys"]
    out = {}
    for shape, side in (("blocks", 8), ("quads", 2), ("sixteens", 4)):
        wave = (ys // side) * (case.w // side) + xs // side
        tally = {"grid": 0, "tree": 0, "full": 0, "outside": 0, "waves": 0}
        for k in np.unique(wave[send]):
            lanes = send & (wave == k)
            tally["waves"] += 1
            (a0, a1), (b0, b1) = cell_span(u[lanes], s, nu, MARGIN), cell_span(v[lanes], s, nv, MARGIN)
            (c0, c1), (d0, d1) = cell_span(u[lanes], s, nu, -MARGIN), cell_span(v[lanes], s, nv, -MARGIN)
            if (a1 - a0 + 1) * (b1 - b0 + 1) <= GRID_WAVE_CELLS:
                tally["grid"] += 1
                tally["full"] += bool((counts[d0:d1 + 1, c0:c1 + 1] > 64).any())
            elif (c1 - c0 + 1) * (d1 - d0 + 1) > GRID_WAVE_CELLS:
                tally["tree"] += 1
            tally["outside"] += bool((lanes & off).any())
        out[shape] = tally
    return out


# ---------------------------------------------------------------------------------------------------------------- the conditions
def assert_shadows_exist(name):
    """On the oracle alone: under some light at least 50 receiver pixels lie in the mesh's shadow, under every light at least 50 are lit;
    and for the meshes that can shadow themselves the same with 20 of the mesh's own pixels."""
    counts = shadow_counts(name)
    case = CASES[name]
    print(f"{name}: per light (receiver shadowed, receiver lit, mesh shadowed, mesh lit) {counts}")
    assert max(c[0] for c in counts.values()) >= 50 and min(c[1] for c in counts.values()) >= 50, (name, counts)
    if len(case.parts) == 1 and case.parts[0][0] in SELF_SHADOWING:
        assert max(c[2] for c in counts.values()) >= 20 and max(c[3] for c in counts.values()) >= 20, (name, counts)


@functools.lru_cache(maxsize=None)
def routes_of(name):
    """route_counts of every pair of the case that has a grid, summed per wave shape."""
    _, nodes, _, _ = structures(name)
    total = {}
    for l, rec in pairs_of(name):
        if grid_of(rec)[2] == 0:
            continue
        for shape, tally in route_counts(name, l, rec, nodes).items():
            for k, v in tally.items():
                total.setdefault(shape, {}).setdefault(k, 0)
                total[shape][k] += v
    return total


def assert_routes_reached(name):
    """At least 8 waves surely through the grid, 8 surely through the tree behind it, 8 with receiver lanes beyond the grid's border and,
    for the meshes with crowded cells, 8 grid waves that visit a cell of more than 64 entries: for the 8x8 blocks a large frame's waves
    are and for the 2x2 squares these frames' waves are on an MI355X."""
    total = routes_of(name)
    print(f"{name}: {total}")
    crowded = CASES[name].parts[0][0] in ("concentric", "geometric")
    for shape in ("blocks", "quads"):
        t = total[shape]
        assert t["grid"] >= 8 and t["tree"] >= 8 and t["outside"] >= 8, (name, shape, t)
        if crowded:
            assert t["full"] >= 8, (name, shape, t)

"""The per-block triangle candidate lists (k_block_lists, mesh_list_closest) against a reference that shares no code with the kernels
(tests/list_tools.py), on the degenerate meshes of tests/bvh_tools.py and on views chosen for the slacks the two culls rest on.

Every GPU case renders its frame with the option off and on (bitwise equal, every counter too), compares it with the oracle's and then
checks the lists Context.block_lists() reads back, for every active block:
  * a listed block:  must <= faces in the list <= may; no face twice; at most 64; every bounded entry's float rectangle contains the exact
    rectangle and lies inside the exact one grown by 2e-3 of its size plus m; entries of unbounded triangles are infinite on all four sides;
  * a block without a list has a reason: |may| > 64, or the pool was full (entries in use + |must| > capacity), or the reference finds its
    pyramid degenerate;
  * the headers do not overlap in the pool and none points past the entries in use.
So that this is not vacuous, the undecided band may \\ must (unbounded triangles left out), summed over a case, holds at most 5 % of |may|
(evaluated on the CPU, test_band_cap_holds_for_every_case) and every case has a listed block with a non-empty must.  Two cases are exempt
by construction and assert their outcome directly: `identical`, from outside and from inside (every block the mesh reaches overflows), and
the edge-on view of `flat` (every rectangle has zero height, and sits on the border between two rows of blocks).  DESIGN.md 15.1 holds the measured band and the share of listed blocks per case."""
import collections
import math

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from oracle import ft_oracle_py as O

from . import bvh_tools as B
from . import helpers as H
from . import list_tools as LT
from .test_block_lists import LIGHTS, counters, wavy, with_filler
from .test_light_space_shadows import built

LD = LT.LD
BAND_CAP = 0.05
Case = collections.namedtuple("Case", "name tris ops cam w h jitter lights expect")
S3 = [("scale", (3.0, 3.0, 3.0))]


def cam_at(o, look, up=(0, 1, 0), fov=60.0, aspect=1.0):
    return ft.make_camera(tuple(float(v) for v in o), tuple(float(v) for v in look), up, math.radians(fov), aspect)


def _moved(tris, z):
    """wavy(6) with the grid vertex at (0, -1/3) moved to z in every triangle that uses it."""
    t = np.array(tris, dtype=np.float64).reshape(-1, 3, 3)
    g = np.linspace(-1.0, 1.0, 7)
    sel = (t[:, :, 0] == g[3]) & (t[:, :, 2] == g[2])
    assert sel.sum() == 6
    t[sel, 2] = z
    return t.reshape(-1, 9)


def _stack(cam, w, h, centres, n, size_px=0.5):
    """n small parallel triangles stacked behind one another on the ray through each pixel position of `centres`."""
    pl = LT.oracle_plane(cam, w, h)
    out = []
    for px, py in centres:
        d = pl.k + (pl.tlx + px * pl.pw) * pl.i - (py * pl.ph - pl.tly) * pl.j
        for k in range(n):
            t = 2.0 + 0.02 * k
            c, s = pl.o + t * d, size_px * pl.pw * t
            out.append(np.concatenate([c + s * (-pl.i - pl.j), c + s * (pl.i - pl.j), c + s * pl.j]))
    return np.array(out)


# Where the quarter-radius rule gives a view without a listable block (or, for `identical`, without the mesh in it): another point inside the bounds.
# chain(256): its 256 equal triangles fill every view that has them in front, so they stay behind and the far corner's triangle is in view.
_U = np.array([1.0, 0.3, 1.0]) / np.linalg.norm([1.0, 0.3, 1.0])
INSIDE = {"identical": (-0.45, -0.2, -0.45), "concentric": (-1.66, 0.1, -0.15), "chain(256)": tuple(1023.5 - 500.0 * _U + np.array([28.3, 0.0, -28.3]))}


def _make_cases():
    cat = B.catalogue()
    dflt = ft.jitter_pattern(4)
    along = _U
    cases = []

    def add(name, tris, ops, cam, w=64, h=48, jitter=None, lights=LIGHTS, expect=None):
        cases.append(Case(name, np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9)), ops, cam, w, h, dflt if jitter is None else np.asarray(jitter, dtype=np.float64), lights, expect))

    # ---- the catalogue, from outside and from inside
    for name in ("blob(8)", "blob(65)", "blob(1025)", "identical", "concentric", "flat", "flat_x", "two_clusters", "spanning", "degenerate", "chain(256)", "geometric"):
        e = cat[name]
        add(f"{name}-out", e.tris, None, B.camera(e.centre, e.radius), expect="overflow" if name == "identical" else None)
        inside = e.centre - 0.25 * e.radius * along                     # inside the mesh's bounds, a quarter of the radius behind their centre
        if name in INSIDE:
            inside = np.array(INSIDE[name])
        add(f"{name}-in", e.tris, None, cam_at(inside, inside + along), expect="overflow" if name == "identical" else None)
    e = cat["geometric"]
    o1 = e.centre + e.radius * np.array([0.9, 1.3, -3.6])
    add("geometric-near", e.tris, None, cam_at(o1 * 16.0 ** -8, o1 * 16.0 ** -8 + (e.centre - o1)))
    # ---- the camera plane
    axis_cam = cam_at((0.25, 0.75, -0.75), (0.25, 0.75, 1.25))               # k = (0, 0, 1), i = (1, 0, 0), j = (0, 1, 0), all exact
    add("plane-a=0", _moved(wavy(6), -0.25), S3, axis_cam)
    add("plane-a=+2^-40", _moved(wavy(6), -0.25 + 2.0 ** -40), S3, axis_cam)
    add("plane-a=-2^-40", _moved(wavy(6), -0.25 - 2.0 ** -40), S3, axis_cam)
    t = 3.0 * wavy(6).reshape(-1, 3, 3)[40]
    add("plane-in-triangle", wavy(6), S3, cam_at(t[0] + 1.75 * (t[1] - t[0]) - 0.5 * (t[2] - t[0]), (0.5, 0.0, 0.5)))
    add("flat-1e-9-above", cat["flat"].tris, None, cam_at((-3.0, 0.25, 0.37 + 1e-9), (0.0, 0.0, 0.57), up=(0, 0, 1)))   # looking up a little: the plane's line off the border between two rows of blocks
    add("flat-edge-on", cat["flat"].tris, None, cam_at((-3.0, 0.25, 0.37), (0.0, 0.0, 0.37), up=(0, 0, 1)), expect="zero_height")
    # ---- transforms of the mesh leaf
    look = (0.13, 0.0, 0.07)                                            # not the mesh's middle vertex: the point looked at lands on a corner of four blocks
    main_cam = cam_at((0.2, 2.5, -3.0), look)
    add("xf-sliver", wavy(6), [("scale", (1e3, 1.0, 1e-3)), ("rotate", (1.0, 2.0, 3.0), 0.7)], cam_at((300.0, 900.0, -1200.0), (40.0, 25.0, 10.0)))   # (the point looked at lands on a corner of four blocks: not the sliver's middle)
    add("xf-mirror", wavy(6), S3 + [("scale", (-1.0, 1.0, 1.0))], main_cam)
    add("xf-shear", wavy(6), [("rotate", (0, 0, 1), 0.6), ("scale", (2.0, 0.5, 1.0)), ("rotate", (0, 0, 1), -0.6)] + S3, main_cam)
    add("xf-flat_x-edge-on", cat["flat_x"].tris, [("rotate", (0, 0, 1), math.pi / 2)], cam_at((0.1, 0.37, -3.0), (0.0, 0.57, 0.0)), lights=[("dir", (1, 0, 0))])   # (looking up a little, as above)
    # ---- field of view, aspect, frame shapes
    far = 1e4 * 4.3 * np.array([0.2, 2.5, -3.0]) / np.linalg.norm([0.2, 2.5, -3.0])
    add("fov-0.5", wavy(4), S3, cam_at(far, (20.0, 0.0, 12.0), fov=0.5))
    add("fov-150", wavy(6), S3, cam_at((0.2, 2.5, -3.0), look, fov=150.0))
    add("aspect-2", wavy(6), S3, cam_at((0.2, 2.5, -3.0), look, aspect=2.0))
    add("aspect-0.5", wavy(6), S3, cam_at((0.2, 2.5, -3.0), look, aspect=0.5))
    add("frame-8x8", wavy(4), S3, main_cam, w=8, h=8)
    add("frame-8x64", wavy(6), S3, main_cam, w=8, h=64)
    add("frame-128x8", wavy(6), S3, cam_at((0.2, 2.5, -3.0), (0.13, -2.5, 0.9)), w=128, h=8)   # (the plane's rows are 1 / 127 of its height: the frame is its top edge)
    pl = LT.oracle_plane(main_cam, 64, 48)
    at = lambda px, py: pl.o + 5.0 * (pl.k + (pl.tlx + px * pl.pw) * pl.i + (pl.tly - py * pl.ph) * pl.j)
    edge = [0.1 * cat["blob(8)"].tris + at(px, py) for px, py in ((12.5, 44.5), (36.5, 44.5), (60.5, 44.5), (60.5, 20.5), (60.5, 4.5))]
    add("last-row-and-column", np.concatenate(edge), None, main_cam)
    # ---- jitter patterns
    add("jitter-corners", wavy(6), S3, main_cam, jitter=[(0, 0), (1, 0), (0, 1), (1, 1)])
    add("jitter-3.5", wavy(6), S3, main_cam, jitter=[(3.5, 3.5), (-3.5, 3.5), (3.5, -3.5), (-3.5, -3.5)])
    add("jitter-64", wavy(4), S3, main_cam, jitter=[(64.0, 0.0), (0, 0), (0.25, -0.25), (-0.5, 0.5)])
    add("jitter-64.5", wavy(4), S3, main_cam, jitter=[(64.5, 0.0), (0, 0), (0.25, -0.25), (-0.5, 0.5)], expect="no_lists")
    add("jitter-16", wavy(6), S3, main_cam, jitter=ft.jitter_pattern(16))
    # ---- the list cap and the pool
    front = cam_at((0, 0, -2), (0, 0, 2))
    few = _stack(front, 64, 48, [(11.5, 11.5)], 3)                        # a second block, which carries a list in both cases
    add("cap-64", with_filler(np.concatenate([_stack(front, 64, 48, [(35.5, 27.5)], 64), few])), None, front, expect="cap64")
    add("cap-65", with_filler(np.concatenate([_stack(front, 64, 48, [(35.5, 27.5)], 65), few])), None, front, expect="cap65")
    # rectangles far below a float's resolution of their coordinates: only the outward rounding keeps what is stored around them
    spots = [(5.3, 4.7), (11.3, 9.7), (50.2, 40.1), (35.5, 27.5), (20.9, 33.3), (60.1, 3.2), (3.4, 44.6), (44.4, 14.8)]
    add("tiny-stacks", with_filler(_stack(front, 64, 48, spots, 6, size_px=1e-9)), None, front)
    add("pool", _stack(front, 128, 96, [(8 * x + 3.5, 8 * y + 3.5) for y in range(12) for x in range(16)], 60), None, front, w=128, h=96, lights=[("dir", (-3, -2, 3))], expect="pool")
    return {c.name: c for c in cases}


CASES = _make_cases()
NAMES = list(CASES)
assert len(NAMES) <= 70
EXEMPT = ("overflow", "zero_height", "no_lists")
_REF, _ORACLE = {}, {}


def ref_of(name):
    """The reference of a case, computed once per session and never modified."""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = LT.reference(c.tris, c.ops, c.cam, c.w, c.h, c.jitter)
    return _REF[name]


def oracle_frame(name):
    if name not in _ORACLE:
        c = CASES[name]
        orc = O.Oracle()
        built(c.tris, c.lights, xf=c.ops)(orc)
        _ORACLE[name] = orc.render(c.cam, c.w, c.h, c.jitter.shape[0], c.jitter)[0]
        orc.close()
    return _ORACLE[name]


# ---------------------------------------------------------------------------------------------------------------- not GPU
def _one(tri, ops, cam, w=64, h=48):
    return LT.reference(np.array([tri], dtype=np.float64), ops, cam, w, h, np.zeros((1, 2)))


def test_reference_on_hand_worked_projections():
    cam = cam_at((0, 0, -2), (0, 0, 2))                                   # k = (0, 0, 1), i = (1, 0, 0), j = (0, 1, 0)
    pl = LT.oracle_plane(cam, 64, 48)
    assert pl.k.tolist() == [0, 0, 1] and pl.i.tolist() == [1, 0, 0] and pl.j.tolist() == [0, 1, 0]
    # square to the camera, 4 in front of it: jx = x / 4, jy = y / 4
    r = _one([[-0.25, -0.125, 2], [0.5, -0.125, 2], [0, 0.375, 2]], None, cam)
    assert (r.a == 4).all() and not r.unbounded[0] and not r.near[0]
    assert (float(r.x0[0]), float(r.x1[0]), float(r.y0[0]), float(r.y1[0])) == (-0.0625, 0.125, -0.03125, 0.09375)
    # its blocks: pixel x = (jx - tlx) / pw, y = (tly - jy) / ph
    px0, px1 = (-0.0625 - pl.tlx) / pl.pw, (0.125 - pl.tlx) / pl.pw
    py0, py1 = (pl.tly - 0.09375) / pl.ph, (pl.tly + 0.03125) / pl.ph
    want = np.zeros((6, 8), dtype=bool)
    for cy in range(6):
        for cx in range(8):
            want[cy, cx] = px1 >= 8 * cx - 1 and px0 <= 8 * cx + 8 and py1 >= 8 * cy - 1 and py0 <= 8 * cy + 8   # the block's pixels +- the extent 1
    assert want.sum() == 4 and np.array_equal(r.must[:, 0].reshape(6, 8), want) and np.array_equal(r.may, r.must) and r.band == 0
    # one vertex behind the camera: unbounded, a candidate of every block, a must only where a sample ray hits it
    r = _one([[-0.25, -0.125, 2], [0.5, -0.125, 2], [0, 0.375, -3]], None, cam)
    assert r.unbounded[0] and r.a[0, 2] == -1 and np.isinf(r.x0[0]) and np.isinf(r.y1[0]) and r.may.all() and r.sampled > 0
    hit = np.zeros(48, dtype=bool)
    for y in range(48):
        for x in range(64):
            hit[(y // 8) * 8 + x // 8] |= _moller([[-0.25, -0.125, 2], [0.5, -0.125, 2], [0, 0.375, -3]], *O.ray_through_pixel(cam, 64, 48, x, y))
    assert 0 < hit.sum() < 48 and np.array_equal(r.must[:, 0], hit)
    # mirrored by a scale of -1: x = 1, 2, 1 at z = 2 lands at jx = -0.25, -0.5
    r = _one([[1, 0, 2], [2, 0, 2], [1, 1, 2]], [("scale", (-1.0, 1.0, 1.0))], cam)
    assert (float(r.x0[0]), float(r.x1[0]), float(r.y0[0]), float(r.y1[0])) == (-0.5, -0.25, 0.0, 0.25)
    # the jitter's sign: the oracle's ray through pixel (5, 7) under the offset (0.25, -0.5) looks through x = 5.25, y = 7.5
    cam2 = cam_at((0.2, 2.5, -3.0), (0, 0, 0))
    o, d = O.ray_through_pixel(cam2, 64, 48, 5, 7, 0.25, -0.5)
    pl2 = LT.oracle_plane(cam2, 64, 48)
    a, jx, jy = LT.project(pl2, (o + 2.5 * d).astype(LD))
    assert abs(float((jx - pl2.tlx) / pl2.pw) - 5.25) < 1e-12 and abs(float((pl2.tly - jy) / pl2.ph) - 7.5) < 1e-12 and abs(float(a) - 2.5) < 1e-12
    # a rotation composed here is the oracle's (Transform.fs:55-71): a quarter turn about z takes x to y
    M = LT.compose([("rotate", (0, 0, 2.0), math.pi / 2), ("translate", (1.0, 0.0, 0.0))])
    assert np.allclose(np.asarray(M @ np.array([1, 0, 0, 1], dtype=LD), dtype=np.float64), [1, 1, 0, 1], atol=1e-15)


def _moller(tri, o, d):
    a, b, c = (np.array(v, dtype=np.float64) for v in tri)
    e1, e2 = b - a, c - a
    hh = np.cross(d, e2)
    det = e1 @ hh
    s = o - a
    u = (s @ hh) / det
    q = np.cross(s, e1)
    v = (d @ q) / det
    return abs(det) > 1e-7 and 0 <= u <= 1 and v >= 0 and u + v <= 1 and (e2 @ q) / det > 1e-7


def _copy(L):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in L.items()}


def test_checker_fails_on_corrupted_lists():
    ref = ref_of("plane-a=-2^-40")                                        # bounded and unbounded triangles in one frame
    tri_src = np.arange(ref.n, dtype=np.uint32)
    good = LT.synthetic_lists(ref)
    rep = LT.check_lists(good, tri_src, ref)
    assert rep["listed_with_must"] > 4 and rep["none"] == 0
    count = (good["heads"] & 127).astype(int)
    first = (good["heads"] >> 7).astype(int)
    # a block with three bounded candidates at least, and one it cannot reach
    blk = next(b for b in range(ref.nbx * ref.nby) if (ref.must[b] & ~ref.unbounded).sum() >= 3)
    at = next(first[blk] + k for k in range(count[blk]) if not ref.unbounded[good["entries"]["orig"][first[blk] + k]])
    # an entry dropped from a block
    bad = _copy(good)
    bad["entries"][at] = good["entries"][first[blk] + count[blk] - 1]
    bad["heads"][blk] = (first[blk] << 7) | (count[blk] - 1)
    with pytest.raises(AssertionError, match="misses faces"):
        LT.check_lists(bad, tri_src, ref)
    # an entry added to a block it cannot reach: the last entry of the block becomes a face outside its may
    bad = _copy(good)
    far = int(np.nonzero(~ref.may[blk] & ref.must.any(axis=0))[0][0])
    other = next(b for b in range(ref.nbx * ref.nby) if ref.must[b, far])
    src = next(first[other] + k for k in range(count[other]) if good["entries"]["orig"][first[other] + k] == far)
    bad["entries"][first[blk] + count[blk] - 1] = good["entries"][src]
    with pytest.raises(AssertionError, match="cannot reach"):
        LT.check_lists(bad, tri_src, ref)
    # a rectangle one float ulp inside the exact one
    f = int(good["entries"]["orig"][at])
    bad = _copy(good)
    bad["entries"]["x0"][at] = np.nextafter(LT.float_below(ref.x0[f:f + 1])[0], np.float32(np.inf))
    assert LD(bad["entries"]["x0"][at]) > ref.x0[f]
    with pytest.raises(AssertionError, match="does not contain the exact one"):
        LT.check_lists(bad, tri_src, ref)
    # a rectangle ten times too wide
    bad = _copy(good)
    w = float(ref.x1[f] - ref.x0[f])
    bad["entries"]["x0"][at], bad["entries"]["x1"][at] = np.float32(float(ref.x0[f]) - 4.5 * w), np.float32(float(ref.x1[f]) + 4.5 * w)
    with pytest.raises(AssertionError, match="wider than the exact one"):
        LT.check_lists(bad, tri_src, ref)
    # a duplicated entry
    bad = _copy(good)
    bad["entries"][at + 1 if at + 1 < first[blk] + count[blk] else at - 1] = good["entries"][at]
    with pytest.raises(AssertionError, match="listed twice"):
        LT.check_lists(bad, tri_src, ref)
    # an unbounded triangle with a finite side
    ub = next(k for k in range(good["entries"].size) if ref.unbounded[good["entries"]["orig"][k]])
    bad = _copy(good)
    bad["entries"]["y1"][ub] = np.float32(1e30)
    with pytest.raises(AssertionError, match="not infinite on all four sides"):
        LT.check_lists(bad, tri_src, ref)
    # kListNone on a block with three candidates
    three = next(b for b in range(ref.nbx * ref.nby) if 3 <= ref.must[b].sum() and ref.may[b].sum() <= LT.LIST_CAP)
    bad = _copy(good)
    bad["heads"][three] = _capi.LIST_NONE
    with pytest.raises(AssertionError, match="no list without a reason"):
        LT.check_lists(bad, tri_src, ref)
    bad["capacity"] = good["entries"].size + 2                            # ... but with the pool that full it has one
    LT.check_lists(bad, tri_src, ref)
    # a header that overlaps its neighbour, and one that points past the entries
    nxt = next(b for b in range(blk + 1, ref.nbx * ref.nby) if count[b])
    bad = _copy(good)
    bad["heads"][nxt] = ((first[nxt] - 1) << 7) | count[nxt]
    with pytest.raises(AssertionError, match="overlap in the pool"):
        LT.check_lists(bad, tri_src, ref)
    last = int(np.argmax(first + count))
    bad = _copy(good)
    bad["heads"][last] = (first[last] + 1 << 7) | count[last]
    with pytest.raises(AssertionError, match="points past"):
        LT.check_lists(bad, tri_src, ref)
    # a list of 65
    big = ref_of("cap-65")
    good65 = LT.synthetic_lists(big)
    blk65 = int(np.argmax(big.may.sum(axis=1)))
    assert good65["heads"][blk65] == _capi.LIST_NONE and big.must[blk65].sum() == 65
    LT.check_lists(good65, np.arange(big.n, dtype=np.uint32), big)


def test_band_cap_holds_for_every_case():
    """The 5 % cap on the undecided band, per case, with the figures DESIGN.md 15.1 lists; and the views are what their names say."""
    print()
    for name in NAMES:
        c, ref = CASES[name], ref_of(name)
        may, must = int(ref.may.sum()), int(ref.must.sum())
        print(f"  {name:24s} {ref.n:6d} triangles  unbounded {int(ref.unbounded.sum()):4d}  near {int(ref.near.sum()):3d}  |must| {must:7d}  |may| {may:7d}  band {ref.band:5d}"
              f" ({ref.band / max(may, 1):.4f})  sampled {ref.sampled:7d}  blocks |may| <= 64 and must: {int(((ref.may.sum(axis=1) <= 64) & ref.must.any(axis=1)).sum())}")
        if c.expect in EXEMPT:
            continue
        assert ref.band <= BAND_CAP * may, f"{name}: the undecided band holds {ref.band} of {may}"
        assert ref.must.any(), f"{name}: no block has a non-empty must"
        if not ref.unbounded.any():
            assert ((ref.may.sum(axis=1) <= LT.LIST_CAP) & ref.must.any(axis=1)).any(), f"{name}: no block can carry a list with a non-empty must"
        assert not ref.degenerate.any(), name
    # exempt by construction
    r = ref_of("identical-out")
    assert ((r.must.sum(axis=1) == 0) | (r.must.sum(axis=1) == 300)).all() and (r.must.sum(axis=1) == 300).any()
    r = ref_of("flat-edge-on")
    assert not r.unbounded.any() and (r.y0 == r.y1).all()
    r = ref_of("xf-flat_x-edge-on")                                       # a quarter turn in binary64 is not exact: heights of rounding size
    assert not r.unbounded.any() and 0 < float((r.y1 - r.y0).max()) < 1e-15
    # the views
    for name, n_ub in (("plane-a=0", 6), ("plane-a=-2^-40", 6)):
        assert int(ref_of(name).unbounded.sum()) >= n_ub
    r0, rp, rm = ref_of("plane-a=0"), ref_of("plane-a=+2^-40"), ref_of("plane-a=-2^-40")
    for r, z, a in ((r0, -0.25, 0.0), (rp, -0.25 + 2.0 ** -40, 3 * 2.0 ** -40), (rm, -0.25 - 2.0 ** -40, -3 * 2.0 ** -40)):
        name = {0.0: "plane-a=0"}.get(a, "plane-a=+2^-40" if a > 0 else "plane-a=-2^-40")
        sel = CASES[name].tris.reshape(-1, 3, 3)[:, :, 2] == z
        assert sel.sum() == 6 and (r.a[sel] == a).all()
        assert r.unbounded[sel.any(axis=1)].all() if a <= 0 else (r.near[sel.any(axis=1)].any() and not r.unbounded[sel.any(axis=1)].all())
    r = ref_of("plane-in-triangle")
    assert r.unbounded.any()
    r = ref_of("last-row-and-column")
    hit = r.must.any(axis=1).reshape(r.nby, r.nbx)
    assert hit[-1, -1] and not hit[:-1, :-1].any()
    r = ref_of("geometric-near")
    tiny = (r.x1 - r.x0) < 6e-8 * np.abs(r.x0)
    assert int((tiny & ~r.unbounded).sum()) >= 64, "the nested triangles project to rectangles below a float's resolution of jx"
    for name, n in (("cap-64", 64), ("cap-65", 65)):
        r = ref_of(name)
        per = r.must.sum(axis=1)
        assert per.max() == n and sorted(per[per > 0]) == [3, n] and np.array_equal(r.may, r.must)
    r = ref_of("tiny-stacks")
    inward = (r.x1.astype(np.float32).astype(LD) < r.x1) | (r.y1.astype(np.float32).astype(LD) < r.y1)
    assert int(inward[:48].sum()) >= 12 and (LT.K_GROW * r.size[:48] < 1e-4 * 6e-8 * np.abs(r.x1[:48])).all(), "a plain cast of the upper edges lands inside the exact rectangle"
    r = ref_of("pool")
    assert (r.must.sum(axis=1) == 60).all() and np.array_equal(r.may, r.must)
    assert 60 * r.nbx * r.nby > 16 * r.nbx * r.nby + 4096                   # d_list_pool (ft_frame.cpp): 16 entries a block + 4096
    assert ref_of("jitter-64").ext == 64.0 and ref_of("jitter-3.5").ext == 3.5 and ref_of("jitter-corners").ext == 1.0


# ---------------------------------------------------------------------------------------------------------------- GPU
def render_both(ctx, c):
    """The case's frame with the lists off and on: equal bit for bit, every counter too."""
    spp = c.jitter.shape[0]
    built(c.tris, c.lights, xf=c.ops)(ctx)
    out = []
    try:
        for opt in (0, 1):
            ctx.set_option("primary_block_lists", opt)
            img, st = ctx.render(c.cam, c.w, c.h, spp, c.jitter)
            out.append((img, counters(st)))
        lists = ctx.block_lists()
    finally:
        ctx.set_option("primary_block_lists", 1)
    (a, sa), (b, sb) = out
    assert np.array_equal(a, b), f"frames differ on {np.count_nonzero(np.any(a != b, axis=2))} pixels"
    assert sa == sb
    return a, sa, lists


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_lists_against_the_reference(hip, name):
    c, ref = CASES[name], ref_of(name)
    frame, st, L = render_both(hip, c)
    err = H.assert_frames_match(frame, oracle_frame(name), what=name)
    if c.expect == "no_lists":
        assert L["leaf"] == -1 and L["heads"].size == 0
        return
    LT.assert_plane_agrees(L["plane"], ref)
    face = hip.mesh_trees()["tri_src"]
    rep = LT.check_lists(L, face, ref)
    print(f"\n  {name}: active {rep['active']} listed {rep['listed']} (with a must: {rep['listed_with_must']}) without {rep['none']} entries {rep['entries']} of {L['capacity']}"
          f" hits {st['hits_primary']} frame error {err:.2e}")
    heads, blocks = L["heads"], L["pos_block"]
    none = heads == _capi.LIST_NONE
    if c.expect == "overflow":                                            # every block the triangles reach overflows
        reached = ref.must[blocks].any(axis=1)
        assert reached.any() and none[reached].all()
    elif c.expect == "zero_height":
        e = L["entries"]
        assert e.size > 0 and rep["listed_with_must"] > 0
        f = face[e["orig"]]                                               # zero height: what is stored is the growth and the margin alone
        assert (e["y1"].astype(LD) - e["y0"].astype(LD) <= 2 * (2 * LT.K_GROW * ref.size[f] + ref.m_ty[f])).all() and (ref.y1[f] - ref.y0[f] < 1e-15).all()
    else:
        assert rep["listed_with_must"] > 0, "no listed block has a non-empty must: the case passes on the walk alone"
    per = {int(b): int(h) for b, h in zip(blocks, heads)}
    if c.expect in ("cap64", "cap65"):
        blk = int(np.argmax(ref.must.sum(axis=1)))
        assert blk in per and st["hits_primary"] > 0
        assert per[blk] == _capi.LIST_NONE if c.expect == "cap65" else (per[blk] != _capi.LIST_NONE and (per[blk] & 127) == 64)
    if c.expect == "pool":
        assert rep["active"] == ref.nbx * ref.nby and L["capacity"] == 16 * rep["active"] + 4096
        assert rep["listed"] == L["capacity"] // 60 and rep["none"] == rep["active"] - rep["listed"]

"""Tools for tests/test_edge_cull.py: a numpy twin of the edge records of option "edge_cull" (functracer_amd/csrc/ft_edges.h: the record
of a projected triangle and the wave-level test made of it), an exact triangle-against-rectangle test in numpy.longdouble that shares
nothing with either, and the inputs of both for the hard-mesh catalogues of tests/list_tools.py (candidate lists: the (jx, jy) of the
image plane) and tests/shadow_tools.py (shadow grids: the (u, v) of a pair's frame).

A record is three lines (a, b, c) as float32; inside is a x + b y + c <= 0; nine zeros are the sentinel, which cuts nothing off.  The twin
follows ft_edges.h operation by operation in float64 (numpy fuses nothing), so it gives the kernel's records where it is given the
kernel's inputs; the tests only rely on the properties, and on the sentinel rule away from its thresholds."""
import numpy as np

from . import list_tools as LT

LD = LT.LD
SLIVER, FLOAT_SLACK, MAX_MARGIN = 2e-6, 1e-6, 5e-3                     # kEdgeSliver, kEdgeFloatSlack, kEdgeMaxMargin


def edge_records(x, y, E, bounded=None):
    """x, y [n, 3] float64: the projected vertices; E [n]: the inflation the entry's rectangle carries; bounded [n].  Returns (records
    [n, 3, 3] float32, info): info holds what the sentinel rule compared - area2 / (SLIVER l2) and m / (MAX_MARGIN size), each > 1 or
    < 1 - so that a test can leave out records a rounding decides."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    E = np.broadcast_to(np.asarray(E, dtype=np.float64), (n,))
    ok = np.ones(n, dtype=bool) if bounded is None else np.asarray(bounded, dtype=bool).copy()
    with np.errstate(all="ignore"):
        ok &= E >= 0.0
        w, h = x.max(axis=1) - x.min(axis=1), y.max(axis=1) - y.min(axis=1)
        X, Y = np.abs(x).max(axis=1) + E, np.abs(y).max(axis=1) + E
        area2 = np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]))
        l2 = np.zeros(n)
        rec = np.zeros((n, 3, 3), dtype=np.float32)
        worst_m = np.zeros(n)
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            ex, ey = x[:, j] - x[:, i], y[:, j] - y[:, i]
            len2 = ex * ex + ey * ey
            l2 = np.fmax(l2, len2)
            ln = np.sqrt(len2)
            a, b = ey / ln, -ex / ln
            flip = a * (x[:, k] - x[:, i]) + b * (y[:, k] - y[:, i]) > 0.0
            a, b = np.where(flip, -a, a), np.where(flip, -b, b)
            af, bf = a.astype(np.float32), b.astype(np.float32)
            a64, b64 = af.astype(np.float64), bf.astype(np.float64)
            d = np.full(n, -np.inf)
            for v in range(3):
                d = np.fmax(d, a64 * x[:, v] + b64 * y[:, v])
            fa, fb = np.abs(a64), np.abs(b64)
            m = (fa + fb) * E + FLOAT_SLACK * ((fa * X + fb * Y) + np.abs(d))
            cd = -(d + m)
            cf = (cd - (2.4e-7 * np.abs(cd) + 1e-37)).astype(np.float32)
            ok &= (m < MAX_MARGIN * (w + h)) & (np.abs(af) + np.abs(bf) + np.abs(cf) < np.float32(3e38))
            worst_m = np.fmax(worst_m, m)
            rec[:, i, 0], rec[:, i, 1], rec[:, i, 2] = af, bf, cf
        ok &= area2 > SLIVER * l2
        rec[~ok] = 0.0
        info = {"area": area2 / (SLIVER * l2), "margin": worst_m / (MAX_MARGIN * (w + h)), "size": w + h}
    return rec, info


def is_sentinel(rec):
    return (np.asarray(rec).reshape(-1, 9) == 0).all(axis=1)


def wave_outside(rec, x0, x1, y0, y1):
    """edges_outside of ft_edges.h in float32: the rectangle lies wholly outside one line of the record.  rec [n, 3, 3]; the rectangle's
    sides scalars or [n]."""
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, 3, 3)
    x0, x1, y0, y1 = (np.broadcast_to(np.asarray(v, dtype=np.float32), (rec.shape[0],)) for v in (x0, x1, y0, y1))
    out = np.zeros(rec.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            a, b, c = rec[:, i, 0], rec[:, i, 1], rec[:, i, 2]
            t = (np.fmin(a * x0, a * x1) + np.fmin(b * y0, b * y1)) + c          # float32 throughout (np.fmin: fminf's NaN rule)
            out |= t > np.float32(0.0)
    return out


def exact_overlap(x, y, x0, x1, y0, y1):
    """A closed triangle against a closed rectangle by the separating axes of both (the rectangle's two, the triangle's three edge
    normals), in longdouble.  x, y [n, 3]; the rectangle's sides [n] or scalars.  A degenerate triangle is the segment or point it is."""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    x0, x1, y0, y1 = (np.broadcast_to(np.asarray(v, dtype=LD), (x.shape[0],)) for v in (x0, x1, y0, y1))
    hit = (x.max(axis=1) >= x0) & (x.min(axis=1) <= x1) & (y.max(axis=1) >= y0) & (y.min(axis=1) <= y1)
    cx, cy = np.stack([x0, x1, x1, x0], axis=1), np.stack([y0, y0, y1, y1], axis=1)
    for i in range(3):
        j = (i + 1) % 3
        nx, ny = y[:, j] - y[:, i], -(x[:, j] - x[:, i])
        t = nx[:, None] * x + ny[:, None] * y
        r = nx[:, None] * cx + ny[:, None] * cy
        hit &= (t.max(axis=1) >= r.min(axis=1)) & (t.min(axis=1) <= r.max(axis=1))
    return hit


def assert_records_hold(rec, x, y, what, beyond=0.01):
    """What the device's records owe the exact projected triangles x, y [n, 3] (longdouble): every vertex inside every line, in float64; and,
    of a record that is not the sentinel, the point `beyond` of the triangle's size (width + height of its rectangle) outside the
    midpoint of each edge lies outside some line.  Returns the number of records that are not the sentinel."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 3, 3)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    live = ~is_sentinel(rec)
    val = rec[:, :, None, 0] * x[:, None, :] + rec[:, :, None, 1] * y[:, None, :] + rec[:, :, None, 2]          # [n, line, vertex]
    bad = live & (val > 0).any(axis=(1, 2))
    assert not bad.any(), f"{what}: a vertex of record {np.nonzero(bad)[0][:5]} lies outside one of its lines"
    size = (x.max(axis=1) - x.min(axis=1)) + (y.max(axis=1) - y.min(axis=1))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        nx, ny = y[:, j] - y[:, i], -(x[:, j] - x[:, i])
        ln = np.hypot(nx, ny)
        with np.errstate(all="ignore"):
            nx, ny = nx / ln, ny / ln
        flip = nx * (x[:, k] - x[:, i]) + ny * (y[:, k] - y[:, i]) > 0
        nx, ny = np.where(flip, -nx, nx), np.where(flip, -ny, ny)
        px, py = 0.5 * (x[:, i] + x[:, j]) + beyond * size * nx, 0.5 * (y[:, i] + y[:, j]) + beyond * size * ny
        out = (rec[:, :, 0] * px[:, None] + rec[:, :, 1] * py[:, None] + rec[:, :, 2] > 0).any(axis=1)
        bad = live & ~out
        assert not bad.any(), f"{what}: the point {beyond} of the size beyond edge {i} of record {np.nonzero(bad)[0][:5]} lies inside every line"
    return int(live.sum())


def assert_sentinels_by_rule(rec, twin, info, what, band=4.0):
    """The device's sentinels against the twin's, wherever neither threshold of the rule lies within a factor `band` of what it compares
    (the twin's inputs are the exact projections, the kernel's carry its own rounding)."""
    with np.errstate(all="ignore"):
        clear = ~((info["area"] > 1 / band) & (info["area"] < band)) & ~((info["margin"] > 1 / band) & (info["margin"] < band))
    got, want = is_sentinel(rec), is_sentinel(twin)
    bad = clear & (got != want)
    assert not bad.any(), f"{what}: records {np.nonzero(bad)[0][:5]}: sentinel on the device {got[bad][:5]}, by the rule {want[bad][:5]}"
    return int((clear & want).sum())


# ------------------------------------------------------------------------------------------------------------ the catalogues' inputs
def list_inputs(ref, tris, ops, cam):
    """Per triangle of a list_tools reference: the exact (jx, jy) of its vertices (longdouble; NaN where unbounded), the inflation its
    entry's rectangle carries (the growth by 1e-3 of its size plus the reference's bound on the kernel's projection error) and bounded."""
    M = LT.compose(ops)
    Pw = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3).astype(LD) @ M[:3, :3].T + M[:3, 3]
    _, jx, jy = LT.project(ref.plane, Pw)
    with np.errstate(invalid="ignore"):
        E = LT.K_GROW * ref.size + np.maximum(ref.m_tx, ref.m_ty) / LT.FACTOR
    return jx, jy, np.asarray(E, dtype=np.float64), ~ref.unbounded


def grid_entries(pairs, nodes, ls_tris, rec_index):
    """The entries of the grid of pair record `rec_index` as ft_debug_light_space hands the arrays out: (record indices into ls_tris
    [m], x, y [m, 3] longdouble: the records' vertices in the pair's (u, v), boxes [m, 5] float32).  Empty where the pair has no grid."""
    P = pairs[rec_index]
    w = P[14:16].view(np.uint32)
    cells, dims = int(w[1]), int(w[3])
    nu, nv = dims & 0xFFFF, dims >> 16
    words = np.asarray(nodes).reshape(-1)
    idx, boxes = [], []
    for c in range(nu * nv):
        first, box, count = (int(v) for v in words[cells + 4 * c:cells + 4 * c + 3])
        idx.append(np.arange(first, first + count))
        boxes.append(words[box:box + 5 * count].view(np.float32).reshape(count, 5))
    if not idx or sum(a.size for a in idx) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=LD), np.zeros((0, 3), dtype=LD), np.zeros((0, 5), dtype=np.float32)
    idx, boxes = np.concatenate(idx), np.concatenate(boxes)
    T = np.asarray(ls_tris, dtype=np.float64).reshape(-1, 9)[idx].astype(LD)
    U, V, c0 = P[0:3].astype(LD), P[3:6].astype(LD), P[9:12].astype(LD)
    verts = np.stack([T[:, 0:3], T[:, 0:3] + T[:, 3:6], T[:, 0:3] + T[:, 6:9]], axis=1) - c0
    return idx, verts @ U, verts @ V, boxes


def grid_inflation(x, y, boxes):
    """How far an entry's box lies outside its projected vertices: the inflation k_ls_edges reads off the box."""
    x, y, b = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(boxes, dtype=np.float64)
    return np.maximum(np.maximum(x.min(axis=1) - b[:, 0], b[:, 1] - x.max(axis=1)), np.maximum(y.min(axis=1) - b[:, 2], b[:, 3] - y.max(axis=1)))


def random_rects(rng, x, y, n, spread):
    """n rectangles per triangle (x, y [m, 3]): centred within `spread` triangle sizes of the triangle's centroid, from a point up to
    a tenth of the size wide - a batch's footprint against a triangle many batches wide.  Returns (triangle index [m n], x0, x1, y0, y1)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = x.shape[0]
    t = np.repeat(np.arange(m), n)
    size = ((x.max(axis=1) - x.min(axis=1)) + (y.max(axis=1) - y.min(axis=1)))[t]
    cx, cy = x.mean(axis=1)[t] + spread * size * rng.uniform(-1, 1, t.size), y.mean(axis=1)[t] + spread * size * rng.uniform(-1, 1, t.size)
    hw, hh = 0.05 * size * rng.uniform(0, 1, t.size) ** 2, 0.05 * size * rng.uniform(0, 1, t.size) ** 2
    return t, cx - hw, cx + hw, cy - hh, cy + hh

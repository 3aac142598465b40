"""Tools for tests/test_block_lists_exact.py: a reference for the per-block triangle candidate lists (k_block_lists) that shares no code
with the kernels, and a checker of what Context.block_lists() reads back.

The reference works in world space and in numpy.longdouble (64 bits of mantissa on x86, asserted below: its own rounding, 1e-19, is
seven orders under the smallest margin), not in fractions.Fraction: a rotation by an angle has no rational matrix, so the transform
would be rounded either way, and the 2.2 M block-triangle pairs of the pool case are one vectorised comparison here.  The mesh's
vertices go through the transform operations the test applied, composed here (`compose`); the camera basis and the image plane come
from the oracle's image_plane.  A vertex p maps to (a, b, c) = [k i j]^-1 (p - o), jx = b / a, jy = c / a; the exact rectangle of a
triangle is the bounding rectangle of its three (jx, jy).  A triangle with any a <= 0 is *unbounded*.

The margin.  k_block_lists (the comment above it in ft_kernels.hip) documents four slacks; m brackets them with a factor of four:
  * round_down / round_up move a value by 2.4e-7 of its magnitude before the cast to float, once for the triangle's rectangle and once
    for the block's: 2 x 2.4e-7 |T| on the triangle's side, 2 x 2.4e-7 |B| on the block's (|T|, |B|: the larger edge magnitude on that axis;
    the cast itself, 6e-8, is inside the second 2.4e-7);
  * the block's rectangle is widened by ext * 1.000001 instead of ext: 1e-6 ext pw (ph on the other axis);
  * every projected quantity carries kProjEps = 1e-12 times the magnitudes that went in, in the leaf's model space: with R the rows of
    [Km Im Jm]^-1, e_a = kProjEps sum_c |R_ac| (|p_c| + |o_c|) and likewise e_b, e_c, and a vertex's jx is off by (e_b + |jx| e_a) / a.
So  m_T = 4 (2 x 2.4e-7 |T| + max over the vertices of (e_b + |jx| e_a) / a),  m_B = 4 (2 x 2.4e-7 |B| + 1e-6 ext pw),  m = m_T + m_B.
The fourth slack, the growth by 1e-3 of the rectangle's size (width + height, as the kernel adds them), is not part of m: `may` and the
tightness check allow twice that growth, 2e-3, beside m.

  must(block): the bounded triangles whose exact rectangle overlaps the block's rectangle shrunk by m.  The kernel keeps them: a node box
      outside one side of the block's pyramid lies outside that side of the rectangle, so the walk reaches every such triangle's leaf.
  may(block):  every unbounded triangle, every triangle with a <= 4 e_a at a vertex (the kernel asks a - e_a > 0: it may call such a
      triangle unbounded), and every bounded triangle whose rectangle, grown by 2e-3 of its size plus m_T, overlaps the block's widened by m_B.
Unbounded triangles join must by sampling: the reference's triangle test (Triangle.fs:43-66) in float64 numpy over every sample ray of
the frame, in the leaf's model space as Transform.fs hands the ray on; a hit whose u, v, u + v, t or determinant lies within 1e-9
relative of its limit decides nothing."""
import types

import numpy as np

from functracer_amd import _capi
from oracle import ft_oracle_py as O

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is no wider than float64 here: the reference needs 64 bits of mantissa"

LIST_CAP = 64                                                        # kListCap
K_PROJ_EPS, K_ROUND, K_EXT, K_GROW = 1e-12, 2.4e-7, 1e-6, 1e-3        # the constants of the comment above k_block_lists
FACTOR = 4.0
NEAR = 1e-9
TRI_EPS = 0.0000001                                                  # Triangle.fs:44


# ------------------------------------------------------------------------------------------------------------ transforms and the plane
def compose(ops):
    """The model-to-world matrix [4, 4] of transform operations as SceneBuilder.transform takes them (first listed applied first)."""
    M = np.eye(4, dtype=LD)
    for op in ops or []:
        T = np.eye(4, dtype=LD)
        v = np.array([float(x) for x in (op[1] if not np.isscalar(op[1]) else (op[1],) * 3)], dtype=LD)
        if op[0] == "translate":
            T[:3, 3] = v
        elif op[0] == "scale":
            T[0, 0], T[1, 1], T[2, 2] = v
        elif op[0] == "rotate":
            u = v / np.sqrt((v * v).sum())
            c, s = np.cos(LD(float(op[2]))), np.sin(LD(float(op[2])))
            K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]], dtype=LD)
            T[:3, :3] = c * np.eye(3, dtype=LD) + (1 - c) * np.outer(u, u) + s * K
        else:
            raise ValueError(op[0])
        M = T @ M
    return M


def inv3(A):
    """The inverse of a 3 x 3 matrix by cofactors (numpy.linalg does not take longdouble)."""
    c = np.array([np.cross(A[1], A[2]), np.cross(A[2], A[0]), np.cross(A[0], A[1])], dtype=LD)
    return c.T / (A[0] * c[0]).sum()


def oracle_plane(cam, w, h):
    ip = O.image_plane(cam, w, h)
    return types.SimpleNamespace(o=np.array(cam.o[:], dtype=np.float64), i=ip["i"], j=ip["j"], k=ip["k"], pw=float(ip["pixel_width"]),
                                 ph=float(ip["pixel_height"]), tlx=float(ip["top_left"][0]), tly=float(ip["top_left"][1]))


def assert_plane_agrees(plane, ref):
    """Context.block_lists()["plane"] against the oracle's, to 1e-12 relative."""
    want = np.array([ref.plane.tlx, ref.plane.tly, ref.plane.pw, ref.plane.ph])
    assert np.all(np.abs(np.asarray(plane) - want) <= 1e-12 * np.abs(want)), (plane, want)


# ------------------------------------------------------------------------------------------------------------ the reference
def project(pl, Pw):
    """(a, jx, jy) of world points Pw[..., 3] (longdouble); jx, jy are NaN where a <= 0."""
    basis = np.array([pl.k, pl.i, pl.j], dtype=LD).T                 # columns k, i, j
    R = inv3(basis)
    abc = (Pw - pl.o.astype(LD)) @ R.T
    a = abc[..., 0]
    safe = np.where(a > 0, a, LD(1))
    jx, jy = np.where(a > 0, abc[..., 1] / safe, LD(np.nan)), np.where(a > 0, abc[..., 2] / safe, LD(np.nan))
    return a, jx, jy


def reference(tris, ops, cam, w, h, jitter, sample_unbounded=True):
    """must / may per 8x8 block of a w x h frame (block b = (y // 8) * (w // 8) + x // 8) for the triangles `tris` [n, 3, 3] in list order
    under `ops`, seen by `cam` with the jitter offsets `jitter` [spp, 2]."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    jitter = np.asarray(jitter, dtype=np.float64).reshape(-1, 2)
    assert w % 8 == 0 and h % 8 == 0
    pl = oracle_plane(cam, w, h)
    ext = max(1.0, float(np.abs(jitter).max()))
    M = compose(ops)
    A, tr = M[:3, :3], M[:3, 3]
    Pw = tris.astype(LD) @ A.T + tr
    a, jx, jy = project(pl, Pw)
    unbounded = (a <= 0).any(axis=1)
    # the kernel's documented error bound, in the leaf's model space
    Ainv = inv3(A)
    om = Ainv @ (pl.o.astype(LD) - tr)
    Rm = inv3(np.array([pl.k, pl.i, pl.j], dtype=LD).T) @ A
    e = K_PROJ_EPS * ((np.abs(tris.astype(LD)) + np.abs(om)) @ np.abs(Rm).T)     # [n, 3, (a, b, c)]
    near = ~unbounded & (a <= FACTOR * e[..., 0]).any(axis=1)
    safe = np.where(a > 0, a, LD(1))
    proj_x = np.where(unbounded, LD(0), np.nanmax(np.where(a > 0, (e[..., 1] + np.abs(jx) * e[..., 0]) / safe, LD(0)), axis=1))
    proj_y = np.where(unbounded, LD(0), np.nanmax(np.where(a > 0, (e[..., 2] + np.abs(jy) * e[..., 0]) / safe, LD(0)), axis=1))
    inf = LD(np.inf)
    with np.errstate(invalid="ignore"):
        x0, x1 = np.where(unbounded, -inf, jx.min(axis=1)), np.where(unbounded, inf, jx.max(axis=1))
        y0, y1 = np.where(unbounded, -inf, jy.min(axis=1)), np.where(unbounded, inf, jy.max(axis=1))
    size = np.where(unbounded, LD(0), (x1 - x0) + (y1 - y0))
    m_tx = np.where(unbounded, LD(0), FACTOR * (2 * K_ROUND * np.maximum(np.abs(x0), np.abs(x1)) + proj_x))
    m_ty = np.where(unbounded, LD(0), FACTOR * (2 * K_ROUND * np.maximum(np.abs(y0), np.abs(y1)) + proj_y))
    # the blocks
    nbx, nby = w // 8, h // 8
    cx, cy = (np.arange(nbx * nby) % nbx).astype(LD), (np.arange(nbx * nby) // nbx).astype(LD)
    tlx, tly, pw, ph = LD(pl.tlx), LD(pl.tly), LD(pl.pw), LD(pl.ph)
    bx0, bx1 = tlx + (8 * cx - ext) * pw, tlx + (8 * cx + 7 + ext) * pw
    by0, by1 = tly - (8 * cy + 7 + ext) * ph, tly - (8 * cy - ext) * ph
    m_bx = FACTOR * (2 * K_ROUND * np.maximum(np.abs(bx0), np.abs(bx1)) + K_EXT * ext * pw)
    m_by = FACTOR * (2 * K_ROUND * np.maximum(np.abs(by0), np.abs(by1)) + K_EXT * ext * ph)
    B = lambda v: v[:, None]
    T = lambda v: v[None, :]
    with np.errstate(invalid="ignore"):
        mx, my = B(m_bx) + T(m_tx), B(m_by) + T(m_ty)
        must = T(~unbounded) & (T(x1) >= B(bx0) + mx) & (T(x0) <= B(bx1) - mx) & (T(y1) >= B(by0) + my) & (T(y0) <= B(by1) - my)
        gx, gy = 2 * K_GROW * size + m_tx, 2 * K_GROW * size + m_ty
        may = T(unbounded | near) | ((T(x1 + gx) >= B(bx0 - m_bx)) & (T(x0 - gx) <= B(bx1 + m_bx)) & (T(y1 + gy) >= B(by0 - m_by)) & (T(y0 - gy) <= B(by1 + m_by)))
    may |= must
    band = int((may & ~must & T(~unbounded)).sum())
    # the pyramid of a block in the leaf's model space: degenerate where a float cannot tell which way a side faces
    degenerate = np.zeros(nbx * nby, dtype=bool)
    corners = [(bx0, by0), (bx1, by0), (bx1, by1), (bx0, by1)]
    dirs = [(np.asarray(pl.k, dtype=LD)[None, :] + B(qx) * np.asarray(pl.i, dtype=LD)[None, :] + B(qy) * np.asarray(pl.j, dtype=LD)[None, :]) @ Ainv.T for qx, qy in corners]
    for c in range(4):
        n = np.cross(dirs[c], dirs[(c + 1) & 3])
        terms = n * dirs[(c + 2) & 3]
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(terms.sum(axis=1)) / np.abs(terms).sum(axis=1)
        degenerate |= ~(rel > 1e-5)
    ref = types.SimpleNamespace(w=w, h=h, nbx=nbx, nby=nby, n=tris.shape[0], plane=pl, ext=ext, a=a, x0=x0, x1=x1, y0=y0, y1=y1, size=size, m_tx=m_tx, m_ty=m_ty,
                                unbounded=unbounded, near=near, must=must, may=may, band=band, degenerate=degenerate, sampled=0)
    if sample_unbounded and unbounded.any():
        ref.sampled = _sample_unbounded(ref, tris, np.asarray(Ainv, dtype=np.float64), np.asarray(om, dtype=np.float64), jitter)
    return ref


def _sample_unbounded(ref, tris, Ainv, om, jitter):
    """Every sample ray of the frame against every unbounded triangle by the reference's own test, in float64; a decided hit puts the triangle
    into must of the pixel's block.  Returns the number of such hits."""
    pl, w, h = ref.plane, ref.w, ref.h
    ys, xs = np.mgrid[0:h, 0:w]
    block = ((ys // 8) * ref.nbx + xs // 8).ravel()
    idx = np.nonzero(ref.unbounded)[0]
    v0, e1, e2 = tris[idx, 0], tris[idx, 1] - tris[idx, 0], tris[idx, 2] - tris[idx, 0]
    s = om[None, :] - v0                                              # [U, 3]
    q = np.cross(s, e1)
    found = 0
    for ox, oy in jitter:                                             # rayThroughPixel, Image.fs:83-89
        jx = ((pl.tlx + xs * pl.pw) + ox * pl.pw).ravel()
        jy = ((pl.tly - ys * pl.ph) + oy * pl.ph).ravel()
        d = (pl.k[None, :] + jx[:, None] * pl.i[None, :] + jy[:, None] * pl.j[None, :]) @ Ainv.T     # [R, 3]
        for lo in range(0, idx.size, 64):
            sl = slice(lo, lo + 64)
            hh = np.cross(d[:, None, :], e2[None, sl, :])             # [R, u, 3]
            det = (e1[None, sl, :] * hh).sum(axis=2)
            with np.errstate(divide="ignore", invalid="ignore"):
                f = 1.0 / det
                u = f * (s[None, sl, :] * hh).sum(axis=2)
                v = f * (d[:, None, :] * q[None, sl, :]).sum(axis=2)
                t = f * (e2[sl] * q[sl]).sum(axis=1)[None, :]
                hit = (np.abs(det) > TRI_EPS * (1 + NEAR)) & (u > NEAR) & (u < 1 - NEAR) & (v > NEAR) & (u + v < 1 - NEAR) & (t > TRI_EPS * (1 + NEAR))
            r, k = np.nonzero(hit)
            ref.must[block[r], idx[lo + k]] = True
            found += r.size
    ref.may |= ref.must
    return found


# ------------------------------------------------------------------------------------------------------------ the checker
def check_lists(lists, tri_src, ref):
    """Assert what the module docstring of tests/test_block_lists_exact.py lists about the lists of one frame.  Returns counts."""
    heads, pos_block, ent, cap = lists["heads"], lists["pos_block"], lists["entries"], int(lists["capacity"])
    assert lists["leaf"] >= 0, "the frame carried no lists"
    assert heads.shape == pos_block.shape
    n_ent = int(ent.shape[0])
    face = np.asarray(tri_src)[ent["orig"]].astype(np.int64)
    sx0, sx1, sy0, sy1 = (ent[k].astype(LD) for k in ("x0", "x1", "y0", "y1"))
    # headers
    spans = sorted((int(hd) >> 7, int(hd) & 127, pos) for pos, hd in enumerate(heads) if hd != _capi.LIST_NONE and (int(hd) & 127))
    for (f0, c0, p0), (f1, _, p1) in zip(spans, spans[1:]):
        assert f0 + c0 <= f1, f"the lists of active blocks {p0} and {p1} overlap in the pool at {f1}"
    for f0, c0, p0 in spans:
        assert f0 + c0 <= n_ent, f"the list of active block {p0} points past the {n_ent} entries"
    n_listed = n_must_listed = n_none = 0
    assert np.unique(pos_block).size == pos_block.size, "a block is active twice"
    for pos, hd in enumerate(int(v) for v in heads):
        b = int(pos_block[pos])
        assert b < ref.nbx * ref.nby, f"active block {pos} is block {b} of {ref.nbx * ref.nby}"
        must, may = ref.must[b], ref.may[b]
        if hd == _capi.LIST_NONE:
            n_none += 1
            why = int(may.sum()) > LIST_CAP or n_ent + int(must.sum()) > cap or bool(ref.degenerate[b])
            assert why, f"block {b} has no list without a reason: |may| {int(may.sum())}, |must| {int(must.sum())}, {n_ent} of {cap} entries used"
            continue
        first, count = hd >> 7, hd & 127
        assert count <= LIST_CAP, f"block {b}: a list of {count}"
        n_listed += 1
        n_must_listed += bool(must.any())
        f = face[first:first + count]
        assert f.size == count and (f < ref.n).all(), f"block {b}: an entry names face {f.max() if f.size else None} of {ref.n}"
        assert np.unique(f).size == count, f"block {b}: a face is listed twice"
        inside = np.zeros(ref.n, dtype=bool)
        inside[f] = True
        missing = np.nonzero(must & ~inside)[0]
        assert missing.size == 0, f"block {b}: the list misses faces {missing[:5]} of must"
        extra = np.nonzero(inside & ~may)[0]
        assert extra.size == 0, f"block {b}: the list holds faces {extra[:5]} that cannot reach it"
        e = slice(first, first + count)
        infinite = np.isinf(sx0[e]) & np.isinf(sx1[e]) & np.isinf(sy0[e]) & np.isinf(sy1[e]) & (sx0[e] < 0) & (sx1[e] > 0) & (sy0[e] < 0) & (sy1[e] > 0)
        assert infinite[ref.unbounded[f]].all(), f"block {b}: the rectangle of an unbounded triangle is not infinite on all four sides"
        chk = ~ref.unbounded[f] & ~(ref.near[f] & infinite)
        fx = f[chk]
        gx0, gx1, gy0, gy1 = sx0[e][chk], sx1[e][chk], sy0[e][chk], sy1[e][chk]
        holds = (gx0 <= ref.x0[fx]) & (gx1 >= ref.x1[fx]) & (gy0 <= ref.y0[fx]) & (gy1 >= ref.y1[fx])
        assert holds.all(), f"block {b}: the stored rectangle of face {fx[~holds][:3]} does not contain the exact one"
        rx, ry = 2 * K_GROW * ref.size[fx] + ref.m_tx[fx], 2 * K_GROW * ref.size[fx] + ref.m_ty[fx]
        tight = (gx0 >= ref.x0[fx] - rx) & (gx1 <= ref.x1[fx] + rx) & (gy0 >= ref.y0[fx] - ry) & (gy1 <= ref.y1[fx] + ry)
        assert tight.all(), f"block {b}: the stored rectangle of face {fx[~tight][:3]} is wider than the exact one grown by 2e-3 of its size plus m"
    return {"active": int(heads.size), "listed": n_listed, "listed_with_must": n_must_listed, "none": n_none, "entries": n_ent}


# ------------------------------------------------------------------------------------------------------------ a synthetic list
def float_below(x):
    """The largest float32 <= x (x: longdouble array)."""
    f = x.astype(np.float32)
    up = f.astype(LD) > x
    f[up] = np.nextafter(f[up], np.float32(-np.inf))
    return f


def float_above(x):
    return -float_below(-x)


def synthetic_lists(ref, capacity=1 << 20):
    """A list as Context.block_lists() returns it, built from the reference: every block active, each listed with its must set and the
    unbounded triangles (kListNone where |may| passes the cap), the rectangles grown by 1e-3 of their size and rounded outward to float.
    tri_src is the identity."""
    heads, rows = [], []
    grow = K_GROW * ref.size
    r = np.zeros(ref.n, dtype=_capi.LIST_ENTRY_DTYPE)
    r["tri"] = r["orig"] = np.arange(ref.n)
    r["x0"], r["x1"], r["y0"], r["y1"] = float_below(ref.x0 - grow), float_above(ref.x1 + grow), float_below(ref.y0 - grow), float_above(ref.y1 + grow)
    for b in range(ref.nbx * ref.nby):
        if int(ref.may[b].sum()) > LIST_CAP:
            heads.append(_capi.LIST_NONE)
            continue
        f = np.nonzero(ref.must[b] | ref.unbounded)[0]
        heads.append((len(rows) << 7) | f.size)
        rows.extend(r[f])
    entries = np.array(rows, dtype=_capi.LIST_ENTRY_DTYPE) if rows else np.zeros(0, dtype=_capi.LIST_ENTRY_DTYPE)
    pl = ref.plane
    return {"leaf": 0, "heads": np.array(heads, dtype=np.uint32), "pos_block": np.arange(ref.nbx * ref.nby, dtype=np.uint32), "entries": entries,
            "plane": np.array([pl.tlx, pl.tly, pl.pw, pl.ph]), "capacity": capacity}

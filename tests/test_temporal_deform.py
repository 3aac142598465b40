"""ft_set_option "temporal_follow_deformed": the temporal history follows the triangles of a mesh that ft_scene_commit_deformed refits.
`taken_back_deformed` restates the definition of include/functracer_hip.h ("history on deforming meshes") / DESIGN.md 16.2 in numpy: a hit
pixel's barycentric coordinates in its live triangle record, the same coordinates in the record the history saw, then the history's pose.
Its inputs come from the public API (render, render_aov with the triangle plane, leaf_matrices) and from the vertices the test itself
set, so it shares no code with k_temporal.  The result feeds test_temporal.py's unchanged restatement, as test_temporal_motion.py's does.

Two expectations differ from the wording of the request this test was written to, because clause 2 of ft_temporal_accumulate compares
WORLD points, not material points:
 - The displacement of the stand-in mesh is 0.9 x extent x (sin(3y / extent) - 0.5) per call, not 0.03 x extent x sin(3y / extent):
   under this camera a pixel is 0.0186 of the depth wide (Image.fs divides the width by res_v - 1), the tolerance of 4 pixel widths is
   0.7 world units at the mesh and the mesh is 1.2 world units tall; the - 0.5 keeps the mesh's middle where the tiles look while its
   ends move apart.  The test asserts from the AOVs that followed points move further than the tolerance.  The case that rebuilds trees
   in place twists the mesh instead (tools/refit_rate.py's deformation, under which the measured cost grows).
 - A planar grid that slides or stretches in its own plane under a static camera shows the SAME world point in a pixel before and after,
   so without the option clause 2 accepts the history of whatever material point was there: N keeps growing where the grid was before
   and starts at 1 only where the grid is new (the strip it slid or stretched over).  That is what the option-0 half of
   test_history_follows_the_grid asserts; with the option N is the number of calls everywhere two pixels inside, new strip included.

The GPU tests print the figures they assert on; what an MI355X gave is in DESIGN.md 16.2 "Measured"."""
import os

import numpy as np
import pytest

import functracer_amd as ft

from . import bvh_tools as B
from . import helpers as H
from .test_mesh_refit import Recorder, deform
from .test_temporal import LEFT_OUT_CAP, TILES, _compare, _mask, image_plane, new_state, orbit, project, ray_through_pixel, reference
from .test_temporal_motion import CALLS, Hh, W, _build, _bunny_tris, _camera, _grown, _matrices, _pose, motion, taken_back

OPTION = "temporal_follow_deformed"
SLIVER = 1e-6                                                        # det < SLIVER * d11 * d22: the solve amplifies fused against unfused sums
AMPLITUDE = 0.9                                                      # of the mesh's extent per call (see the module's docstring)


# ---------------------------------------------------------------------------------------------------------------- the definition, in numpy
def records(tris):
    """The list-order records of a mesh's vertices [n, 3, 3] (a, b, c): (v0, e1 = b - a, e2 = c - a) as 9 doubles, the flattener's subtraction."""
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], axis=1))


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _affine(M, v):
    return np.stack([M[..., i, 0] * v[..., 0] + M[..., i, 1] * v[..., 1] + M[..., i, 2] * v[..., 2] + M[..., i, 3] for i in range(3)], axis=-1)


def _transposed(M, g):
    return np.stack([M[..., 0, j] * g[..., 0] + M[..., 1, j] * g[..., 1] + M[..., 2, j] * g[..., 2] for j in range(3)], axis=-1)


def _candidates(leaf, triangle, first_global, n_tris):
    l = np.clip(leaf, 0, None)
    tau = triangle.astype(np.int64)
    cand = (leaf >= 0) & (tau >= 0) & (tau < np.asarray(n_tris, dtype=np.int64)[l])     # 0 <= tau < n, compared unsigned
    return cand, l, np.where(cand, np.asarray(first_global, dtype=np.int64)[l] + tau, 0)


def _gram(T):
    e1, e2 = T[..., 3:6], T[..., 6:9]
    d11, d12, d22 = _dot3(e1, e1), _dot3(e1, e2), _dot3(e2, e2)
    return d11, d12, d22, d11 * d22 - d12 * d12


def taken_back_deformed(p, n, leaf, triangle, live_records, snapshot_records, W, H, Wh, first_global, n_tris):
    """(pr, nr, followed): p and n [h, w, 3] of the hit pixels on a changed triangle of a snapshotted mesh taken back to where that
    material point was when the history was written; the others as they are.  live_records / snapshot_records: [R, 9], record
    first_global[l] + triangle of leaf l; W, H, Wh: [leaves, 3, 4], the live w2m and the history's m2w and w2m; n_tris[l]: triangles of
    leaf l's snapshot, 0 for a leaf without one."""
    cand, l, idx = _candidates(leaf, triangle, first_global, n_tris)
    T, O = np.ascontiguousarray(live_records[idx]), np.ascontiguousarray(snapshot_records[idx])
    changed = (T.view(np.int64) != O.view(np.int64)).any(axis=-1)
    with np.errstate(all="ignore"):
        r = _affine(W[l], p) - T[..., 0:3]
        e1, e2 = T[..., 3:6], T[..., 6:9]
        d11, d12, d22, det = _gram(T)
        r1, r2 = _dot3(r, e1), _dot3(r, e2)
        beta, gamma = (d22 * r1 - d12 * r2) / det, (d11 * r2 - d12 * r1) / det
        followed = cand & changed & (det > 0.0) & np.isfinite(beta) & np.isfinite(gamma)
        q_old = O[..., 0:3] + beta[..., None] * O[..., 3:6] + gamma[..., None] * O[..., 6:9]
        pr = _affine(H[l], q_old)
        c = _transposed(W[l], _cross(e1, e2))
        s = np.where(_dot3(n, c) < 0.0, -1.0, 1.0)
        t = _transposed(Wh[l], _cross(O[..., 3:6], O[..., 6:9]))
        nr = s[..., None] * t * (1.0 / np.sqrt(_dot3(t, t)))[..., None]
    return np.where(followed[..., None], pr, p), np.where(followed[..., None], nr, n), followed


def sliver_pixels(leaf, triangle, live_records, snapshot_records, first_global, n_tris, **_):
    """Pixels whose triangle is a sliver in either record: what the comparison with the device leaves out."""
    cand, _, idx = _candidates(leaf, triangle, first_global, n_tris)
    out = np.zeros(leaf.shape, dtype=bool)
    for rec in (live_records, snapshot_records):
        d11, _, d22, det = _gram(rec[idx])
        out |= cand & ~(det >= SLIVER * d11 * d22)
    return out


def reference_deforming(prev, plane, c, p, n, leaf, triangle, in_tiles, D, A, moved, deformed=None, **kw):
    """One ft_temporal_accumulate after meshes deformed (and perhaps moved): the pixels that follow a triangle take that way back, the
    others the moved leaf's or none; clauses 1 to 3 run on the result and clause 6 stores the current p, n, leaf."""
    pr, nr = taken_back(p, n, leaf, D, A, moved)
    followed, thin = np.zeros(leaf.shape, dtype=bool), np.zeros(leaf.shape, dtype=bool)
    if deformed is not None:
        pd, nd, followed = taken_back_deformed(p, n, leaf, triangle, **deformed)
        pr, nr = np.where(followed[..., None], pd, pr), np.where(followed[..., None], nd, nr)
        thin = sliver_pixels(leaf, triangle, **deformed)
    st = reference(prev, plane, c, pr, nr, leaf, in_tiles, **kw)
    h3 = (in_tiles & (leaf >= 0))[..., None]
    st["p"], st["n"] = np.where(h3, p, 0.0), np.where(h3, n, 0.0)
    st["taint"] = st["taint"] | (thin & in_tiles)
    return st, pr, followed


def _eye(n=1):
    m = np.zeros((n, 3, 4))
    m[:, :, :3] = np.eye(3)
    return m


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_names_the_option_and_a_host_only_context_takes_it():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert '"temporal_follow_deformed"' in hdr
    ctx = ft.Context(host_only=True)
    for v in (0, 1, 7, 0):                                           # a flag: any other value than 0 means 1
        ctx.set_option(OPTION, v)
    with pytest.raises(ft.FtError) as e:
        ctx.set_option(OPTION + "_", 1)
    assert e.value.status == -1 and "unknown option" in str(e.value)
    ctx.close()


def _one(v):
    return np.asarray(v, dtype=np.float64).reshape(1, 1, -1)


def test_restatement_on_hand_worked_cases():
    tight = dict(rtol=1e-14, atol=1e-14)
    a, b, c = np.array([1.0, 2.0, 3.0]), np.array([3.0, 2.5, 3.0]), np.array([1.5, 4.0, 3.5])
    tri = np.stack([a, b, c])[None]
    live = records(tri)
    e1, e2 = b - a, c - a
    point = a + 0.25 * e1 + 0.5 * e2
    normal = np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2))
    leaf, tau = np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.int32)
    ident = dict(W=_eye(), H=_eye(), Wh=_eye(), first_global=[0], n_tris=[1])
    # identity leaf, the triangle translated by v since the history was written: the point was at p - v, the normal is the same
    v = np.array([0.3, -0.2, 0.1])
    pr, nr, fol = taken_back_deformed(_one(point), _one(normal), leaf, tau, live, records(tri - v), **ident)
    assert fol.all() and np.allclose(pr[0, 0], point - v, **tight) and np.allclose(nr[0, 0], normal, **tight)
    # scaled by 2 about a: the point at (beta, gamma) = (0.25, 0.5) of the live triangle maps to a + 0.25 e1' + 0.5 e2'
    snap = np.stack([a, a + 0.5 * e1, a + 0.5 * e2])[None]           # the history saw the triangle at half the size
    pr, nr, fol = taken_back_deformed(_one(point), _one(normal), leaf, tau, live, records(snap), **ident)
    assert fol.all() and np.allclose(pr[0, 0], a + 0.25 * (0.5 * e1) + 0.5 * (0.5 * e2), **tight) and np.allclose(nr[0, 0], normal, **tight)
    # a point off the triangle's plane (slightOffset) has the coordinates of its foot
    pr2, _, _ = taken_back_deformed(_one(point + 1e-3 * normal), _one(normal), leaf, tau, live, records(snap), **ident)
    assert np.allclose(pr2[0, 0], pr[0, 0], rtol=0, atol=1e-12)
    # a leaf under scale + rotate whose pose changed too (H != m2w), the model-space triangle translated by t: pr = H (W p - t)
    ang = 0.4
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ np.diag([2.0, 0.5, 1.5])
    m2w = np.zeros((1, 3, 4))
    m2w[0, :, :3], m2w[0, :, 3] = R, [4.0, -1.0, 2.0]
    w2m = np.zeros((1, 3, 4))
    w2m[0, :, :3], w2m[0, :, 3] = np.linalg.inv(R), -np.linalg.inv(R) @ m2w[0, :, 3]
    Hm = np.zeros((1, 3, 4))
    Hm[0, :, :3], Hm[0, :, 3] = R @ np.diag([1.0, 1.0, -1.0])[[0, 2, 1]], [3.0, 0.0, 2.5]     # another linear part and another place
    Whm = np.zeros((1, 3, 4))
    Whm[0, :, :3], Whm[0, :, 3] = np.linalg.inv(Hm[0, :, :3]), -np.linalg.inv(Hm[0, :, :3]) @ Hm[0, :, 3]
    t = np.array([0.05, 0.02, -0.04])
    world = m2w[0, :, :3] @ point + m2w[0, :, 3]
    n_world = np.linalg.inv(R).T @ normal
    n_world /= np.linalg.norm(n_world)
    pr, nr, fol = taken_back_deformed(_one(world), _one(n_world), leaf, tau, live, records(tri - t), W=w2m, H=Hm, Wh=Whm, first_global=[0], n_tris=[1])
    want = Hm[0, :, :3] @ ((w2m[0, :, :3] @ world + w2m[0, :, 3]) - t) + Hm[0, :, 3]
    n_then = np.linalg.inv(Hm[0, :, :3]).T @ normal
    n_then /= np.linalg.norm(n_then)
    assert fol.all() and np.allclose(pr[0, 0], want, rtol=1e-13, atol=1e-13)
    assert np.allclose(nr[0, 0], n_then, rtol=1e-13, atol=1e-13) and np.dot(n_world, np.linalg.inv(R).T @ normal) > 0
    # a back-face pixel: n(x) against c, s = -1, nr on the same side of the old triangle
    pr, nr, fol = taken_back_deformed(_one(point), _one(-normal), leaf, tau, live, records(tri - v), **ident)
    assert fol.all() and np.allclose(nr[0, 0], -normal, **tight)
    # the snapshot wound the other way: s is the side of the live triangle n(x) is on, and nr is that same side of the material - of the
    # snapshot's e1' x e2', which points the other way in space
    swapped = np.stack([a, c, b])[None] - v
    for side in (1.0, -1.0):
        pr, nr, fol = taken_back_deformed(_one(point), _one(side * normal), leaf, tau, live, records(swapped), **ident)
        assert fol.all() and np.allclose(nr[0, 0], -side * normal, **tight)    # s belongs to the live winding, t to the snapshot's
        assert np.allclose(pr[0, 0], swapped[0, 0] + 0.25 * (swapped[0, 1] - swapped[0, 0]) + 0.5 * (swapped[0, 2] - swapped[0, 0]), **tight)
    # det = 0 (a collapsed live triangle): not followed, p and n untouched
    flat = np.stack([a, b, a + 2.0 * e1])[None]
    pr, nr, fol = taken_back_deformed(_one(point), _one(normal), leaf, tau, records(flat), records(tri), **ident)
    assert not fol.any() and np.array_equal(pr[0, 0], point) and np.array_equal(nr[0, 0], normal)
    assert sliver_pixels(leaf, tau, records(flat), records(tri), [0], [1]).all() and not sliver_pixels(leaf, tau, live, records(tri - v), [0], [1]).any()
    # bitwise equal records: not followed
    pr, nr, fol = taken_back_deformed(_one(point), _one(normal), leaf, tau, live, live.copy(), **ident)
    assert not fol.any() and np.array_equal(pr[0, 0], point)
    # tau = -1 and tau = n: not followed; nor a leaf without a snapshot, nor a miss pixel
    for bad in (-1, 1):
        _, _, fol = taken_back_deformed(_one(point), _one(normal), leaf, np.full((1, 1), bad, dtype=np.int32), live, records(tri - v), **ident)
        assert not fol.any()
    _, _, fol = taken_back_deformed(_one(point), _one(normal), leaf, tau, live, records(tri - v), **dict(ident, n_tris=[0]))
    assert not fol.any()
    miss = np.full((1, 1), -1, dtype=np.int32)
    pr, nr, fol = taken_back_deformed(_one(point), _one(normal), miss, miss, live, records(tri - v), **ident)
    assert not fol.any() and np.array_equal(pr[0, 0], point) and np.array_equal(nr[0, 0], normal)
    # first_global: the record is looked up at first_global[l] + tau
    two = np.concatenate([records(tri + 9.0), live])
    pr, _, fol = taken_back_deformed(_one(point), _one(normal), leaf, tau, two, np.concatenate([records(tri + 9.0), records(tri - v)]), **dict(ident, first_global=[1]))
    assert fol.all() and np.allclose(pr[0, 0], point - v, **tight)


def _shape(t, amplitude=AMPLITUDE):
    """The stand-in mesh at time t (in calls): x += amplitude * t * extent * (sin(3 y / extent) - 0.5)."""
    v = np.array(_bunny_tris(), dtype=np.float64).reshape(-1, 3, 3)
    extent = float(np.ptp(v.reshape(-1, 3), axis=0).max())
    v[..., 0] += amplitude * t * extent * (np.sin(3.0 * v[..., 1] / extent) - 0.5)
    return v


TWIST = 2.4                                                          # radians per call between the mesh's bottom and its top


def _twisted(t):
    """The stand-in mesh twisted about the vertical axis through its middle, TWIST * t between bottom and top."""
    v = np.array(_bunny_tris(), dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    c = 0.5 * (lo + hi)
    ang = TWIST * t * (v[..., 1] - lo[1]) / (hi[1] - lo[1])
    x, z = v[..., 0] - c[0], v[..., 2] - c[2]
    return np.stack([c[0] + np.cos(ang) * x + np.sin(ang) * z, v[..., 1], c[2] - np.sin(ang) * x + np.cos(ang) * z], axis=-1)


def test_no_triangle_of_the_deformed_mesh_is_a_sliver():
    """From the mesh file alone: under every shape the device test commits, det >= SLIVER * d11 * d22 for all 980 triangles."""
    worst = 1.0
    for half in range(2 * CALLS - 1):
        for shape in (_shape, _twisted):
            d11, _, d22, det = _gram(records(shape(0.5 * half)))
            worst = min(worst, float((det / (d11 * d22)).min()))
    print(f"smallest det / (d11 d22) over the shapes: {worst:.3e}")
    assert worst >= 10.0 * SLIVER


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
@pytest.fixture
def following(hip):
    """The session's context; whatever a test set, the options this file touches go back to their defaults."""
    yield hip
    for key, value in ((OPTION, 0), ("refit_rebuild_percent", 0), ("bvh_builder", 2)):
        hip.set_option(key, value)


def _aov(ctx, cam, spp, jit, sample, seed, tiles=None, w=W, h=Hh):
    return ctx.render_aov(cam, w, h, spp, jit, sample=sample, seed=seed, tiles=tiles, channels=["p", "n", "leaf", "triangle"])


def _deformed(n_leaves, mesh_leaf, now_verts, then_verts, now, then):
    n_tris = np.zeros(n_leaves, dtype=np.int64)
    n_tris[mesh_leaf] = records(now_verts).shape[0]
    return dict(live_records=records(now_verts), snapshot_records=records(then_verts), W=now[1], H=then[0], Wh=then[1],
                first_global=np.zeros(n_leaves, dtype=np.int64), n_tris=n_tris)


def _mesh_leaf(ctx, cam):
    g = _aov(ctx, cam, 1, np.zeros((1, 2)), 0, 1)
    ids = np.unique(g["leaf"][g["triangle"] >= 0])
    assert ids.size == 1, ids
    return int(ids[0])


def _fetch_bits(ctx):
    return tuple(ctx.temporal_fetch()) + (ctx.temporal_status(),)


def _same_runs(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


# ---------------------------------------------------------------------------------------------------------------- 3. device against restatement
def _parity(hip, path, spp, tiles, mode, _shape=_shape):
    rec = Recorder(hip)
    hd = _build(rec, _pose(0.0))
    mesh = rec.meshes[0]
    hip.set_option(OPTION, 1)
    cams = orbit(_camera(), CALLS) if path == "orbit" else [_camera()] * CALLS
    jit, sample = ft.jitter_pattern(spp), spp - 1
    inside = _mask(tiles)
    mesh_leaf = _mesh_leaf(hip, cams[0])
    n_leaves = hip.scene_info()["leaves"]
    hip.temporal_begin(W, Hh, tiles=tiles)
    st, pose_of_set = new_state(Hh, W), None
    worst, share, with_history, followed_px, far = 0.0, 0.0, [], [], 0
    for k, cam in enumerate(cams):
        if k > 0:
            if mode == "two-commits":
                hip.set_mesh_triangles(mesh, _shape(k - 0.5))         # a shape no accumulate ever sees
                hip.commit_deformed()
            if mode == "moved" and k % 2:
                hip.set_transform(hd["mesh"], _pose(float(k))["mesh"])
                hip.commit_moved()
            hip.set_mesh_triangles(mesh, _shape(float(k)))
            hip.commit_deformed()
            if mode == "moved" and not k % 2:
                hip.set_transform(hd["mesh"], _pose(float(k))["mesh"])
                hip.commit_moved()
        c, _ = hip.render(cam, W, Hh, spp, jit, seed=100 + k)
        g = _aov(hip, cam, spp, jit, sample, 100 + k, tiles=tiles)
        out, _ = hip.temporal_accumulate(cam, spp, jit, sample=sample, seed=100 + k, out=np.full((Hh, W, 3), 7.0))
        now = _matrices(hip)
        then = pose_of_set or now
        D, A, moved = motion(now[0], now[1], *then)
        assert int(moved.sum()) == (1 if mode == "moved" and k > 0 else 0)
        deformed = _deformed(n_leaves, mesh_leaf, _shape(float(k)), _shape(float(k - 1)), now, then) if k > 0 else None
        before = st
        st, pr, followed = reference_deforming(st, image_plane(cam, W, Hh), c, g["p"], g["n"], g["leaf"], g["triangle"], inside, D, A, moved, deformed)
        pose_of_set = now
        left_out = int(st["taint"].sum())
        share = max(share, left_out / int(inside.sum()))
        err, M, _, _ = _compare(hip, st, inside & ~st["taint"], f"deform {mode} {path} x{spp} call {k}")
        worst = max(worst, err)
        assert np.array_equal(out[inside], M[inside]) and (out[~inside] == 7.0).all()
        status = hip.temporal_status()
        assert status["calls"] == k + 1 and abs(status["with_history"] - int(st["history"].sum())) <= left_out
        with_history.append(status["with_history"])
        followed_px.append(int((inside & followed & st["history"]).sum()))
        if k > 0:
            assert (followed[inside] == ((g["leaf"] == mesh_leaf) & (g["triangle"] >= 0))[inside]).all()   # every triangle moved
            # how far the deformation alone took the followed points, against clause 2's tolerance: over the whole frame (the tiles show
            # the mesh's middle, which stays)
            f = g if tiles is None else _aov(hip, cam, spp, jit, sample, 100 + k)
            back, _, fol = taken_back_deformed(f["p"], f["n"], f["leaf"], f["triangle"], **deformed)
            back = np.where(fol[..., None], back, taken_back(f["p"], f["n"], f["leaf"], D, A, moved)[0])
            rigid, _ = taken_back(f["p"], f["n"], f["leaf"], D, A, moved)
            pl = before["plane"]
            _, _, zc = project(pl, back)
            far += int((fol & (np.sqrt(((back - rigid) ** 2).sum(-1)) > 4.0 * max(pl["pw"], pl["ph"]) * zc)).sum())
    print(f"temporal deform parity {mode} {path} x{spp} {'tiles' if tiles else 'frame'}: worst error {worst:.3e} x the bound, left out {share:.5%} of the tile pixels, "
          f"pixels with history per call {with_history}, of them on followed triangles {followed_px}, followed pixels moved past the tolerance {far}")
    assert share <= LEFT_OUT_CAP, f"{share:.5%} of the tile pixels are left out"
    assert with_history[0] == 0 and min(followed_px[1:]) > 0 and far > 0
    hip.temporal_end()
    return mesh


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["one-commit", "two-commits", "moved"])
@pytest.mark.parametrize("tiles", [None, TILES], ids=["frame", "tiles"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("path", ["static", "orbit"])
def test_device_matches_the_restatement(following, path, spp, tiles, mode):
    _parity(following, path, spp, tiles, mode)


@pytest.mark.gpu
def test_device_matches_the_restatement_across_rebuilds_in_place(following):
    following.set_option("bvh_builder", 3)
    following.set_option("refit_rebuild_percent", 100)
    mesh = _parity(following, "orbit", 1, None, "one-commit", _shape=_twisted)
    q = following.tree_quality(mesh)
    print(f"rebuilds in place during the sequence: {q['rebuilds']}, cost now / as last built {q['ratio']:.4f}")
    assert q["rebuildable"] == 1 and q["rebuilds"] >= 1


# ---------------------------------------------------------------------------------------------------------------- 4. it follows the surface
GRID_CAM = dict(o=(0.0, 0.0, -10.0), look_at=(0.0, 0.0, 0.0))
GRID_DEPTH = 10.0


def _grid_camera():
    return ft.make_camera(GRID_CAM["o"], GRID_CAM["look_at"], (0.0, 1.0, 0.0), H.deg(50.0), 16.0 / 9.0)


def _grid(pl, x0, x1, y0, y1, quads=16):
    """A planar grid of quads x quads quads (two triangles each) facing the camera at GRID_DEPTH, its corners at the pixel coordinates given."""
    xs, ys = np.linspace(x0, x1, quads + 1), np.linspace(y0, y1, quads + 1)
    at = lambda x, y: pl["o"] + GRID_DEPTH * ray_through_pixel(pl, np.float64(x), np.float64(y))
    tris = []
    for j in range(quads):
        for i in range(quads):
            a, b, c, d = at(xs[i], ys[j]), at(xs[i + 1], ys[j]), at(xs[i + 1], ys[j + 1]), at(xs[i], ys[j + 1])
            tris += [[a, b, c], [a, c, d]]
    return np.array(tris)


def _grid_shape(pl, case, k):
    if case == "slide":                                              # 8 pixel widths per call along the image's x axis
        return _grid(pl, 20.3 + 8.0 * k, 80.3 + 8.0 * k, 25.3, 65.3)
    half = 50.0 * (1.0 + 0.1 * k)                                    # stretched about its centre by 10 % per call in x
    return _grid(pl, 79.7 - half, 79.7 + half, 25.3, 65.3)


def _grid_run(hip, case, option):
    cam, jit = _grid_camera(), np.zeros((1, 2))
    pl = image_plane(cam, W, Hh)
    assert np.array_equal(pl["i"], [1.0, 0.0, 0.0]) and np.array_equal(pl["k"], [0.0, 0.0, 1.0])
    hip.clear()
    mesh = hip.bsp_mesh(0, _grid_shape(pl, case, 0).reshape(-1, 9))
    hip.set_objects(hip.group([hip.material(mesh, colour=(0.9, 0.3, 0.2), apply_lighting=False)]))
    hip.add_directional((0.0, -1.0, 1.0), (1.0, 1.0, 1.0))
    hip.commit()
    hip.set_option(OPTION, option)
    hip.temporal_begin(W, Hh)
    out = []
    for k in range(CALLS):
        if k > 0:
            hip.set_mesh_triangles(mesh, _grid_shape(pl, case, k))
            hip.commit_deformed()
        c, _ = hip.render(cam, W, Hh, 1, jit, seed=400 + k)
        g = _aov(hip, cam, 1, jit, 0, 400 + k)
        hip.temporal_accumulate(cam, 1, jit, seed=400 + k, fetch=False)
        M, _, N = hip.temporal_fetch()
        out.append(dict(c=c, g=g, M=M, N=N, status=hip.temporal_status()))
    hip.temporal_end()
    return pl, out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["slide", "stretch"])
def test_history_follows_the_grid(following, case):
    """An unlit planar grid of 512 triangles facing a static camera slides 8 pixel widths per call, or stretches by 10 % per call.  With
    the option, two pixels inside its silhouette the history length is the number of calls.  Without it (the same sequence on the same
    context) the history is that of the pixel, not of the surface: it starts at 1 wherever the grid is new (see the module's docstring)."""
    pl, on = _grid_run(following, case, 1)
    _, off = _grid_run(following, case, 0)
    ident = (_eye(), _eye())
    fresh_total = 0
    for k in range(CALLS):
        g = on[k]["g"]
        assert all(np.array_equal(g[name], off[k]["g"][name]) for name in ("p", "n", "leaf", "triangle")) and np.array_equal(on[k]["c"], off[k]["c"], equal_nan=True)
        inner = ~_grown(g["leaf"] != 0, 2)
        N, M = on[k]["N"], on[k]["M"]
        assert inner.sum() > 100
        assert (np.abs(N[inner] - (k + 1)) <= 1e-12 * (k + 1)).all(), f"call {k}: N two inside the silhouette is {N[inner].min()!r} .. {N[inner].max()!r}"
        assert np.allclose(M[inner], on[k]["c"][inner], rtol=1e-12, atol=0)
        if k == 0:
            continue
        # the material points behind the pixels, by the restatement: how far they moved, and which pixels the grid did not cover before
        deformed = _deformed(1, 0, _grid_shape(pl, case, k), _grid_shape(pl, case, k - 1), ident, ident)
        pr, _, followed = taken_back_deformed(g["p"], g["n"], g["leaf"], g["triangle"], **deformed)
        fx, _, _ = project(pl, pr)
        xs = np.broadcast_to(np.arange(W, dtype=np.float64), (Hh, W))
        shift = np.abs(fx - xs)
        assert followed[inner].all() and on[k]["status"]["with_history"] >= int(inner.sum())
        fresh = inner & ~_grown(on[k - 1]["g"]["leaf"] == 0, 1)       # more than a pixel from what the grid covered before: no tap finds its leaf
        fresh_total += int(fresh.sum())
        Noff = off[k]["N"]
        print(f"temporal deform follow {case} call {k + 1}: {int(inner.sum())} pixels two inside the grid, material points moved {float(shift[inner].min()):.2f} .. "
              f"{float(shift[inner].max()):.2f} pixel widths; option 0: N {float(Noff[inner].min())} .. {float(Noff[inner].max())}, {int(fresh.sum())} pixels on new ground")
        assert (Noff[fresh] == 1.0).all() and (shift[fresh] > 4.0).all()
        assert (Noff[inner & ~fresh] >= 1.0).all()
        if case == "slide":
            assert np.allclose(shift[inner], 8.0, rtol=0, atol=1e-6)
    assert fresh_total > 100


# ---------------------------------------------------------------------------------------------------------------- 5. one deformation, two routes
def _rigid(k):
    """The model-space motion of call k: a rotation by 3 degrees x k about y through the mesh's middle, then a translation."""
    a = H.deg(3.0 * k)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    centre = np.array([-0.0168, 0.11, -0.0015])
    return R, centre, np.array([0.004 * k, 0.002 * k, 0.0])


@pytest.mark.gpu
def test_vertices_and_transform_give_the_same_history(following):
    """The same rigid motion of the mesh, once written into its vertices (commit_deformed, the option on) and once prepended to its
    transform node (commit_moved): the two scenes differ by the rounding of the vertices, the histories must agree."""
    cam, jit = _camera(), np.zeros((1, 2))
    base = np.array(_bunny_tris(), dtype=np.float64).reshape(-1, 3, 3)
    everywhere = _mask(None)
    pl = image_plane(cam, W, Hh)
    other = ft.Context(device=0)
    try:
        rec = Recorder(following)
        _build(rec, _pose(0.0))
        mesh = rec.meshes[0]
        hd_b = _build(other, _pose(0.0))
        following.set_option(OPTION, 1)
        mesh_leaf, n_leaves = _mesh_leaf(following, cam), following.scene_info()["leaves"]
        following.temporal_begin(W, Hh)
        other.temporal_begin(W, Hh)
        verts = [base]
        st = [new_state(Hh, W), new_state(Hh, W)]
        pose_b = None
        compared = 0
        for k in range(CALLS):
            if k > 0:
                R, centre, t = _rigid(k)
                verts.append((base - centre) @ R.T + centre + t)
                following.set_mesh_triangles(mesh, verts[k])
                following.commit_deformed()
                prepended = [("translate", tuple(-centre)), ("rotate", (0.0, 1.0, 0.0), H.deg(3.0 * k)), ("translate", tuple(centre + t))]
                other.set_transform(hd_b["mesh"], prepended + _pose(0.0)["mesh"])
                other.commit_moved()
            got = []
            for which, ctx in enumerate((following, other)):
                c, _ = ctx.render(cam, W, Hh, 1, jit, seed=600 + k)
                g = _aov(ctx, cam, 1, jit, 0, 600 + k)
                ctx.temporal_accumulate(cam, 1, jit, seed=600 + k, fetch=False)
                _, _, N = ctx.temporal_fetch()
                now = _matrices(ctx)
                if which == 0:
                    D, A, moved = motion(now[0], now[1], *now)
                    deformed = _deformed(n_leaves, mesh_leaf, verts[k], verts[k - 1], now, now) if k > 0 else None
                else:
                    D, A, moved = motion(now[0], now[1], *(pose_b or now))
                    deformed, pose_b = None, now
                st[which], _, _ = reference_deforming(st[which], pl, c, g["p"], g["n"], g["leaf"], g["triangle"], everywhere, D, A, moved, deformed)
                got.append(dict(leaf=g["leaf"], N=N))
            a, b = got
            where = ~_grown(a["leaf"] != b["leaf"], 2) & ~st[0]["taint"] & ~st[1]["taint"]
            diff = np.abs(a["N"] - b["N"])
            on_mesh = where & (a["leaf"] == mesh_leaf)
            print(f"temporal deform two routes call {k + 1}: {int(where.sum())} pixels compared ({int(on_mesh.sum())} on the mesh), worst |N_a - N_b| {float(diff[where].max()):.3e}, "
                  f"with history {int((a['N'][where] > 1).sum())} / {int((b['N'][where] > 1).sum())}, on the mesh {int((a['N'][on_mesh] > 1).sum())}")
            assert np.array_equal(a["N"][where] > 1.0, b["N"][where] > 1.0)
            assert (diff[where] <= 1e-6).all()
            if k > 0:
                compared += int((a["N"][on_mesh] > 1).sum())
        assert compared > 100
    finally:
        other.close()
        following.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 6. what did not change
def _reset(hip, mesh, verts):
    """The mesh back at `verts`, outside any accumulation (so no snapshot is taken)."""
    hip.set_mesh_triangles(mesh, verts)
    hip.commit_deformed()


def _sequence(hip, mesh, option, shape_of, calls=4, seed=700, between=None, aovs=None):
    """begin, `calls` x (commit the shape of the call, render, accumulate); what the accumulation holds after every call (aovs: a list
    that receives every call's surface planes)."""
    cam, jit = _camera(), np.zeros((1, 2))
    if shape_of is not None:
        _reset(hip, mesh, shape_of(0))
    hip.set_option(OPTION, option)
    hip.temporal_begin(W, Hh)
    out = []
    for k in range(calls):
        if k > 0 and shape_of is not None:
            hip.set_mesh_triangles(mesh, shape_of(k))
            hip.commit_deformed()
        if between is not None:
            between(k)
        hip.render(cam, W, Hh, 1, jit, seed=seed + k, fetch=False)
        if aovs is not None:
            aovs.append(_aov(hip, cam, 1, jit, 0, seed + k))
        hip.temporal_accumulate(cam, 1, jit, seed=seed + k, fetch=False)
        out.append(_fetch_bits(hip))
    hip.temporal_end()
    return out


@pytest.mark.gpu
def test_what_did_not_change_gets_the_same_bits(following):
    hip = following
    rec = Recorder(hip)
    _build(rec, _pose(0.0))
    mesh = rec.meshes[0]
    cam, jit = _camera(), np.zeros((1, 2))
    # the same vertices committed again every call: option 1, option 0 and no commit at all are the same accumulation
    plain = _sequence(hip, mesh, 0, None)
    runs = [_sequence(hip, mesh, option, lambda k: _shape(0.0)) for option in (0, 1)]
    for run in runs:
        assert all(_same_runs(x, y) for x, y in zip(run, plain))
    assert plain[-1][3]["with_history"] > 0
    # only the upper half of the mesh is displaced: the rest of the frame does not notice the option
    base = _shape(0.0)
    upper = base[:, :, 1].min(axis=1) > 0.11

    def half(k):
        v = base.copy()
        v[upper] = _shape(0.2 * k)[upper]
        return v
    aovs = []
    off, on = _sequence(hip, mesh, 0, half, seed=720), _sequence(hip, mesh, 1, half, seed=720, aovs=aovs)
    mesh_leaf = _mesh_leaf(hip, cam)
    # With a camera that stands still a pixel's taps lie in its 3x3 neighbourhood of the previous set.  dirty: the pixels of a set that may
    # differ between the two runs - those on displaced triangles, and those that could tap a dirty pixel of the set before.
    dirty = np.zeros((Hh, W), dtype=bool)
    differ, checked_other, checked_same = 0, 0, 0
    for k in range(1, len(on)):
        g, before = aovs[k], aovs[k - 1]
        on_mesh = (g["leaf"] == mesh_leaf) & (g["triangle"] >= 0)
        displaced = on_mesh & upper[np.clip(g["triangle"], 0, None)]
        other = (g["leaf"] != mesh_leaf) & ~_grown(before["leaf"] == mesh_leaf, 1)
        same_tri = on_mesh & ~displaced & ~_grown(dirty, 1)
        for where in (other, same_tri):
            assert all(np.array_equal(x[where], y[where], equal_nan=True) for x, y in zip(on[k][:3], off[k][:3])), f"call {k}"
        checked_other += int(other.sum())
        checked_same += int(same_tri.sum())
        differ += int((on[k][2] != off[k][2]).sum())
        dirty = (_grown(dirty, 1) & (g["leaf"] == mesh_leaf)) | displaced
    print(f"temporal deform untouched: {checked_other} pixels on other leaves, {checked_same} on undisplaced triangles bit-identical; N differs on {differ} pixels elsewhere")
    assert checked_other > W * Hh and checked_same > 20 and differ > 0
    # render, render_aov and the tree quality do not depend on the option
    answers = []
    for option in (0, 1):
        hip.set_option(OPTION, option)
        frame, _ = hip.render(cam, W, Hh, 2, ft.jitter_pattern(2), seed=9)
        g = hip.render_aov(cam, W, Hh, 2, ft.jitter_pattern(2), sample=1, seed=9)
        q = hip.tree_quality(mesh)
        answers.append([frame] + [g[name] for name in ("t", "p", "n", "colour", "material", "leaf", "node", "triangle")] + [np.array([q["cost"], q["cost_built"], q["rebuilds"]])])
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*answers))


# ---------------------------------------------------------------------------------------------------------------- 7. lifecycle
@pytest.mark.gpu
def test_lifecycle(following):
    hip = following
    rec = Recorder(hip)
    _build(rec, _pose(0.0))
    mesh = rec.meshes[0]
    cam, jit = _camera(), np.zeros((1, 2))
    shape = lambda k: _shape(float(k))
    off = _sequence(hip, mesh, 0, shape, seed=800)
    on = _sequence(hip, mesh, 1, shape, seed=800)
    print(f"temporal deform lifecycle: pixels with history after the last call, option 1 / 0: {on[-1][3]['with_history']} / {off[-1][3]['with_history']}")
    assert not _same_runs(on[-1], off[-1]) and on[-1][3]["with_history"] > off[-1][3]["with_history"]
    # the option set to 0 between the commit and the accumulate: the snapshot is dropped, the call is the option-0 run's
    run = _sequence(hip, mesh, 1, shape, seed=800, between=lambda k: hip.set_option(OPTION, 0 if k == 1 else 1), calls=2)
    assert _same_runs(run[1], off[1])
    # after an accumulate the snapshot is gone: a further accumulate with no new commit is the same call of a run whose option was 0 from then on
    tails = []
    for later in (1, 0):
        _reset(hip, mesh, shape(0))
        hip.set_option(OPTION, 1)
        hip.temporal_begin(W, Hh)
        for k in range(3):
            if k == 1:
                hip.set_mesh_triangles(mesh, shape(1))
                hip.commit_deformed()
            if k == 2:
                hip.set_option(OPTION, later)
            hip.render(cam, W, Hh, 1, jit, seed=800 + k, fetch=False)
            hip.temporal_accumulate(cam, 1, jit, seed=800 + k, fetch=False)
            if k == 1:
                assert _same_runs(_fetch_bits(hip), on[1])
        tails.append(_fetch_bits(hip))
        hip.temporal_end()
    assert _same_runs(*tails)
    # temporal_end / temporal_begin between the commit and the accumulate start a fresh accumulation
    _reset(hip, mesh, shape(0))
    hip.set_option(OPTION, 1)
    hip.temporal_begin(W, Hh)
    hip.render(cam, W, Hh, 1, jit, seed=810, fetch=False)
    hip.temporal_accumulate(cam, 1, jit, seed=810, fetch=False)
    hip.set_mesh_triangles(mesh, shape(2))
    hip.commit_deformed()
    hip.temporal_end()
    hip.temporal_begin(W, Hh)
    hip.render(cam, W, Hh, 1, jit, seed=811, fetch=False)
    hip.temporal_accumulate(cam, 1, jit, seed=811, fetch=False)
    M, _, N = hip.temporal_fetch()
    frame = hip.fetch_frame(np.zeros((Hh, W, 3)))
    status = hip.temporal_status()
    assert status["calls"] == 1 and status["with_history"] == 0 and (N[np.isfinite(frame).all(-1)] == 1.0).all() and np.array_equal(M, frame, equal_nan=True)
    # a call that fails before it runs keeps the snapshot: the next good call follows
    hip.set_mesh_triangles(mesh, shape(3))
    hip.commit_deformed()
    with pytest.raises(ft.FtError) as e:
        hip.temporal_accumulate(cam, 1, jit, seed=812, max_history=0)
    assert e.value.status == -1
    hip.render(cam, W, Hh, 1, jit, seed=812, fetch=False)
    hip.temporal_accumulate(cam, 1, jit, seed=812, fetch=False)
    followed_run = _fetch_bits(hip)
    hip.temporal_end()
    # ... against the same two calls with the option 0, and with the option 1 and no failed call in between
    twins = []
    for option in (0, 1):
        _reset(hip, mesh, shape(2))
        hip.set_option(OPTION, option)
        hip.temporal_begin(W, Hh)
        hip.render(cam, W, Hh, 1, jit, seed=811, fetch=False)
        hip.temporal_accumulate(cam, 1, jit, seed=811, fetch=False)
        hip.set_mesh_triangles(mesh, shape(3))
        hip.commit_deformed()
        hip.render(cam, W, Hh, 1, jit, seed=812, fetch=False)
        hip.temporal_accumulate(cam, 1, jit, seed=812, fetch=False)
        twins.append(_fetch_bits(hip))
        hip.temporal_end()
    assert _same_runs(followed_run, twins[1]) and not _same_runs(followed_run, twins[0])
    # a commit refused on the host (an edited mesh of depth > 0) leaves everything as it was, and the next accumulate runs
    hip.clear()
    flat_mesh = hip.bsp_mesh(0, _shape(0.0).reshape(-1, 9))
    deep = hip.bsp_mesh(2, B.catalogue()["blob(63)"].tris.reshape(-1, 9))
    hip.set_objects(hip.group([hip.transform(_pose(0.0)["mesh"], flat_mesh), hip.transform([("translate", (2.0, 1.0, 0.0))], deep), hip.primitive(ft.PLANE)]))
    hip.add_directional((0.4, -1.0, 0.6), (1.0, 1.0, 1.0))
    hip.commit()
    refused = []
    for refuse in (False, True):                                     # (the refused edit stays pending in the graph: it comes last)
        hip.set_option(OPTION, 1)
        hip.temporal_begin(W, Hh)
        hip.render(cam, W, Hh, 1, jit, seed=820, fetch=False)
        hip.temporal_accumulate(cam, 1, jit, seed=820, fetch=False)
        hip.set_mesh_triangles(flat_mesh, _shape(0.5))
        hip.commit_deformed()
        if refuse:
            hip.set_mesh_triangles(deep, B.catalogue()["blob(63)"].tris * 1.01)
            with pytest.raises(ft.FtError) as e:
                hip.commit_deformed()
            assert e.value.status == -4
        hip.render(cam, W, Hh, 1, jit, seed=821, fetch=False)
        hip.temporal_accumulate(cam, 1, jit, seed=821, fetch=False)
        refused.append(_fetch_bits(hip))
        hip.temporal_end()
        if not refuse:
            hip.set_mesh_triangles(flat_mesh, _shape(0.0))
            hip.commit_deformed()
    assert _same_runs(*refused) and refused[0][3]["with_history"] > 0
    # ft_scene_commit still ends the accumulation
    hip.temporal_begin(W, Hh)
    hip.render(cam, W, Hh, 1, jit, seed=830, fetch=False)
    hip.temporal_accumulate(cam, 1, jit, seed=830, fetch=False)
    hip.commit()
    hip.render(cam, W, Hh, 1, jit, seed=831, fetch=False)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_accumulate(cam, 1, jit, seed=831)
    assert e.value.status == -5 and "ft_temporal_begin" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- 8. degenerate meshes
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["collapse", "jitter"])
@pytest.mark.parametrize("name", ["degenerate", "identical", "flat", "two_clusters"])
def test_degenerate_meshes_are_followed_without_harm(following, name, how):
    """The det, finiteness and range guards on real data: every call returns FT_OK (the wrapper raises otherwise), finite frame pixels
    have finite M and Q and N >= 1, the counts stay within the tile pixels."""
    hip = following
    e = B.catalogue()[name]
    cam, jit = B.camera(e.centre, 2.0 * e.radius), np.zeros((1, 2))
    hip.clear()
    mesh = hip.bsp_mesh(0, e.tris.reshape(-1, 9))
    hip.set_objects(hip.group([hip.material(mesh, colour=(0.9, 0.5, 0.2), shineyness=4.0)]))
    hip.add_directional((1, -2, 1), (1, 1, 1))
    hip.commit()
    hip.set_option(OPTION, 1)
    hip.temporal_begin(W, Hh)
    for k in range(3):
        if k > 0:
            hip.set_mesh_triangles(mesh, deform(e, how, amount=float(k))[0])
            hip.commit_deformed()
        frame, _ = hip.render(cam, W, Hh, 1, jit, seed=900 + k)
        hip.temporal_accumulate(cam, 1, jit, seed=900 + k, fetch=False)
        M, se, N = hip.temporal_fetch()
        fin = np.isfinite(frame).all(-1)
        status = hip.temporal_status()
        assert np.isfinite(M[fin]).all() and np.isfinite(se[fin]).all() and (N[fin] >= 1.0).all(), f"call {k}"
        assert status["calls"] == k + 1 and 0 <= status["with_history"] <= W * Hh and 0 <= status["at_max_history"] <= W * Hh
    hip.temporal_end()

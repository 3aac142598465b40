"""ft_sg_set_transform / ft_scene_commit_moved (Context.set_transform / commit_moved): rigid objects of a committed scene are moved
without ending ft_temporal_*, and the history follows each moved leaf.  `reference_moving` extends test_temporal.py's numpy restatement
by the arithmetic of include/functracer_hip.h ("moving rigid objects") / DESIGN.md 14: a moved leaf's point and normal are taken back to
the pose the history was written in, the unchanged restatement is asked about them, and the current point and normal are stored.  Its
inputs come from the public API (render, render_aov, leaf_matrices), so it shares no code with k_temporal.

ft_debug_scene_info refuses an edited graph (as it always has), so "the old commit is still there" after a refused commit_moved is shown
by ft_debug_leaf_matrices, which reads the scene the context holds, and by scene_info answering as it did before the refused call.

The GPU tests print the figures they assert on; what an MI355X gave is in DESIGN.md 14 "Measured"."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import helpers as H
from .test_temporal import (LEFT_OUT_CAP, TILES, _compare, _mask, _surfaces, image_plane, new_state, orbit, project, ray_through_pixel,
                            reference)
from .test_temporal_filter import PARAMS as FILTER_PARAMS
from .test_temporal_filter import _compare as _filter_compare
from .test_temporal_filter import _inputs as _filter_inputs
from .test_temporal_filter import reference as filter_reference

W, Hh = 160, 90
CALLS = 6


# ---------------------------------------------------------------------------------------------------------------- the definition, in numpy
def motion(m2w, w2m, H_, Wh):
    """Per leaf (D, A, moved) of a scene whose leaves stand at (m2w, w2m) [leaves, 3, 4] now and stood at (H_, Wh) when the history was
    written: D = H o w2m as a 3x4 affine product, A = m2w_lin . Wh_lin, moved = any double of m2w differs from H."""
    D = np.zeros_like(m2w)
    for j in range(4):
        D[:, :, j] = H_[:, :, 0] * w2m[:, 0, j, None] + H_[:, :, 1] * w2m[:, 1, j, None] + H_[:, :, 2] * w2m[:, 2, j, None]
    D[:, :, 3] = D[:, :, 3] + H_[:, :, 3]
    A = np.zeros((m2w.shape[0], 3, 3))
    for j in range(3):
        A[:, :, j] = m2w[:, :, 0] * Wh[:, 0, j, None] + m2w[:, :, 1] * Wh[:, 1, j, None] + m2w[:, :, 2] * Wh[:, 2, j, None]
    moved = (np.ascontiguousarray(m2w).view(np.int64) != np.ascontiguousarray(H_).view(np.int64)).any(axis=(1, 2))
    return D, A, moved


def taken_back(p, n, leaf, D, A, moved):
    """(pr, nr): p and n [h, w, 3] of the hit pixels whose leaf moved taken back to the history's pose; the others as they are."""
    l = np.clip(leaf, 0, None)
    mv = (leaf >= 0) & moved[l]
    Dl, Al = D[l], A[l]
    with np.errstate(all="ignore"):
        pr = np.stack([Dl[..., i, 0] * p[..., 0] + Dl[..., i, 1] * p[..., 1] + Dl[..., i, 2] * p[..., 2] + Dl[..., i, 3] for i in range(3)], axis=-1)
        t = np.stack([Al[..., 0, j] * n[..., 0] + Al[..., 1, j] * n[..., 1] + Al[..., 2, j] * n[..., 2] for j in range(3)], axis=-1)
        nr = t * (1.0 / np.sqrt(t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1] + t[..., 2] * t[..., 2]))[..., None]
    return np.where(mv[..., None], pr, p), np.where(mv[..., None], nr, n)


def reference_moving(prev, plane, c, p, n, leaf, in_tiles, D, A, moved, **kw):
    """One ft_temporal_accumulate after the scene moved: clauses 1 to 3 on (pr, nr), clause 6 stores the current p, n, leaf."""
    pr, nr = taken_back(p, n, leaf, D, A, moved)
    st = reference(prev, plane, c, pr, nr, leaf, in_tiles, **kw)
    h3 = (in_tiles & (leaf >= 0))[..., None]
    st["p"], st["n"] = np.where(h3, p, 0.0), np.where(h3, n, 0.0)
    return st


def _translation(v):
    m = np.zeros((1, 3, 4))
    m[0, :, :3], m[0, :, 3] = np.eye(3), v
    return m


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_the_motion_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"int32_t ft_sg_set_transform\(ft_context\* ctx, ft_node node, const ft_transform\* ts, int32_t n\);", hdr)
    assert re.search(r"int32_t ft_scene_commit_moved\(ft_context\* ctx\);", hdr)
    assert re.search(r"int32_t ft_debug_leaf_matrices\(ft_context\* ctx, int64_t\* n_leaves, double\* m2w, double\* w2m\);", hdr)
    assert "#define FT_ABI_VERSION 2" in hdr
    lib = C.CDLL(ft.HIP_LIB)
    for name in ("ft_sg_set_transform", "ft_scene_commit_moved", "ft_debug_leaf_matrices"):
        assert hasattr(lib, name), name
    for name in ("set_transform", "commit_moved", "leaf_matrices"):
        assert callable(getattr(ft.Context, name)) and not hasattr(_capi.SceneBuilder, name), name   # not on the builder the oracle shares


def _small_mesh():
    return np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 0, 1], [1, 0, 1], [0.5, 1, 1]]], dtype=np.float64)


POSES = [dict(inner=[("rotate", (0, 1, 0), 0.3)], outer=[("translate", (1, 2, 3))], operand=[("translate", (0.2, 0.1, 0.0))],
              mesh=[("rotate", (1, 0, 0), 0.1), ("translate", (-2, 0, 1))], deep=[("scale", (1.0, 2.0, 1.0))]),
         dict(inner=[("rotate", (0, 1, 0), 0.7), ("scale", (1.5, 1.0, 0.5))], outer=[("translate", (1.5, 2, 2.5))], operand=[("translate", (0.3, -0.1, 0.2))],
              mesh=[("translate", (-2.5, 0.25, 1))], deep=[("scale", (1.0, 2.5, 1.0)), ("rotate", (0, 0, 1), 0.2)])]


def _build_small(ctx, pose):
    """A cube under two nested transform nodes, a CSG subtract whose second operand moves, a `bspMesh 0` leaf and a BSP-compiled mesh."""
    ctx.clear()
    hd = {}
    hd["inner"] = ctx.transform(pose["inner"], ctx.primitive(ft.CUBE))
    hd["outer"] = ctx.transform(pose["outer"], hd["inner"])
    hd["operand"] = ctx.transform(pose["operand"], ctx.primitive(ft.SPHERE))
    csg = ctx.subtract(ctx.primitive(ft.CUBE), hd["operand"])
    hd["mesh"] = ctx.transform(pose["mesh"], ctx.bsp_mesh(0, _small_mesh()))
    hd["deep"] = ctx.transform(pose["deep"], ctx.bsp_mesh(2, _small_mesh()))
    ctx.set_objects(ctx.group([hd["outer"], csg, hd["mesh"], hd["deep"], ctx.primitive(ft.PLANE)]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    return hd


def _same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


def test_set_transform_refuses_bad_arguments_and_changes_nothing():
    ctx = ft.Context(host_only=True)
    hd = _build_small(ctx, POSES[0])
    old = ctx.leaf_matrices()
    lib = ft.hip_lib()
    one = _capi.transform_array([("translate", (9, 9, 9))])
    bad = _capi.transform_array([("translate", (9, 9, 9)), ("scale", 2.0)])
    bad[1].kind = 3
    not_a_transform = 0                                               # the first node: the cube primitive
    assert lib.ft_sg_set_transform(None, hd["inner"], one, 1) == -1
    assert lib.ft_sg_set_transform(ctx._ctx, -1, one, 1) == -1 and lib.ft_sg_set_transform(ctx._ctx, 10_000, one, 1) == -1
    assert lib.ft_sg_set_transform(ctx._ctx, not_a_transform, one, 1) == -1
    assert lib.ft_sg_set_transform(ctx._ctx, hd["inner"], None, 1) == -1
    assert lib.ft_sg_set_transform(ctx._ctx, hd["inner"], one, 0) == -1 and lib.ft_sg_set_transform(ctx._ctx, hd["inner"], one, -2) == -1
    assert lib.ft_sg_set_transform(ctx._ctx, hd["inner"], bad, 2) == -1           # the second kind is bad: the first is not applied either
    bad[1].kind = -1
    assert lib.ft_sg_set_transform(ctx._ctx, hd["inner"], bad, 2) == -1
    with pytest.raises(ft.FtError) as e:
        ctx.set_transform(hd["inner"], [])
    assert e.value.status == -1
    ctx.commit_moved()                                               # the refused calls were no structural change, and no change at all
    assert _same_bits(ctx.leaf_matrices(), old)
    ctx.commit()
    assert _same_bits(ctx.leaf_matrices(), old)
    ctx.close()


def test_commit_moved_needs_a_commit_and_an_unchanged_structure():
    ctx = ft.Context(host_only=True)
    lib = ft.hip_lib()
    assert lib.ft_scene_commit_moved(None) == -1
    assert lib.ft_scene_commit_moved(ctx._ctx) == -5                 # nothing committed yet
    n = C.c_int64()
    assert lib.ft_debug_leaf_matrices(ctx._ctx, C.byref(n), None, None) == -5 and lib.ft_debug_leaf_matrices(ctx._ctx, None, None, None) == -1
    ctx.set_objects(ctx.group([ctx.primitive(ft.SPHERE)]))
    assert lib.ft_scene_commit_moved(ctx._ctx) == -5                 # built, still not committed

    def info(c):
        try:
            return c.scene_info()
        except ft.FtError as e:
            return e.status

    for change in ("node", "light", "root", "clear"):
        hd = _build_small(ctx, POSES[0])
        old, old_info = ctx.leaf_matrices(), ctx.scene_info()
        ctx.commit_moved()                                           # fine so far
        if change == "node":
            ctx.primitive(ft.CONE)                                   # not even part of the objects
        elif change == "light":
            ctx.add_directional((1, -1, 0), (1, 0, 0))
        elif change == "root":
            ctx.set_objects(ctx.group([hd["outer"]]))
        else:
            ctx.clear()
        before = info(ctx)
        with pytest.raises(ft.FtError) as e:
            ctx.commit_moved()
        assert e.value.status == -5 and "ft_scene_commit" in str(e.value), change
        assert info(ctx) == before and before == -5                  # scene_info answers as before the refused call: the graph is not committed
        assert _same_bits(ctx.leaf_matrices(), old), change          # ... and the scene the context holds is the old commit
        if change != "clear":
            if change == "root":
                ctx.set_objects(ctx.group([hd["outer"], hd["mesh"], hd["deep"]]))
            ctx.commit()                                             # a full commit takes the change
            assert (ctx.scene_info() != old_info) == (change == "root")   # (scene_info counts neither lights nor unused nodes)
            ctx.commit_moved()                                       # ... and moves are possible again
    # ft_set_option is no structural change
    hd = _build_small(ctx, POSES[0])
    old = ctx.leaf_matrices()
    ctx.set_option("csg_mesh_capacity", 48)
    ctx.set_option("chunk_samples", 1 << 20)
    ctx.commit_moved()
    assert _same_bits(ctx.leaf_matrices(), old) and ctx.scene_info()["csg_capacity"] > 0
    ctx.close()


def test_moved_matrices_equal_a_fresh_commit_bit_for_bit():
    a, b = ft.Context(host_only=True), ft.Context(host_only=True)
    hd = _build_small(a, POSES[0])
    first, info = a.leaf_matrices(), a.scene_info()
    assert first[0].shape == (info["leaves"], 3, 4) and info["leaves"] >= 6
    for name, ops in POSES[1].items():                               # other counts of transforms than the nodes were made with, too
        a.set_transform(hd[name], ops)
    with pytest.raises(ft.FtError) as e:                             # the graph is uncommitted, as after every builder call
        a.scene_info()
    assert e.value.status == -5 and _same_bits(a.leaf_matrices(), first)
    a.commit_moved()
    _build_small(b, POSES[1])
    assert a.scene_info() == b.scene_info() and a.scene_info()["leaves"] == info["leaves"]
    assert _same_bits(a.leaf_matrices(), b.leaf_matrices()) and not _same_bits(a.leaf_matrices(), first)
    m2w, w2m = a.leaf_matrices()
    for k in range(m2w.shape[0]):                                    # they are a pair
        full, inv = np.vstack([m2w[k], [0, 0, 0, 1]]), np.vstack([w2m[k], [0, 0, 0, 1]])
        assert np.allclose(full @ inv, np.eye(4), atol=1e-12)
    moved = (m2w != first[0]).any(axis=(1, 2))
    assert moved.sum() >= 4 and not moved.all()                      # the cube, the operand, both meshes; not the CSG's first operand or the plane
    for name, ops in POSES[0].items():                               # and back again
        a.set_transform(hd[name], ops)
    a.commit_moved()
    assert _same_bits(a.leaf_matrices(), first)
    a.close(), b.close()


def test_restatement_on_hand_worked_cases():
    rng = np.random.default_rng(5)
    h, w = 5, 9
    cam = ft.make_camera((1, 2, -7), (0.5, 0, 3), (0, 1, 0), H.deg(50), 1.3)
    pl = image_plane(cam, w, h)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    on = np.ones((h, w), dtype=bool)
    tight = dict(rtol=1e-12, atol=0)
    depth = 5.0
    p = pl["o"] + depth * ray_through_pixel(pl, xs, ys)              # a fronto-parallel patch: every pixel's point lies at zc = depth
    n = np.broadcast_to(-pl["k"], p.shape).copy()
    leaf = np.zeros((h, w), dtype=np.int32)
    frames = [rng.uniform(0.1, 1.0, (h, w, 3)) for _ in range(2)]
    ident = _translation((0, 0, 0))
    first = reference(new_state(h, w), pl, frames[0], p, n, leaf, on)
    for sign in (1.0, -1.0):
        # the patch slides by exactly 3 pixel widths along i: pixel x now shows the point that was 3 columns to the left (right)
        shift = sign * 3.0 * depth * pl["pw"] * pl["i"]
        D, A, moved = motion(_translation(shift), _translation(-shift), ident, ident)
        assert moved.all() and np.allclose(D[0, :, 3], -shift, **tight) and np.array_equal(A[0], np.eye(3))
        pr, nr = taken_back(p, n, leaf, D, A, moved)
        fx, fy, zc = project(pl, pr)
        assert np.abs(fx - (xs - sign * 3.0)).max() < 1e-9 and np.abs(fy - ys).max() < 1e-9 and np.allclose(zc, depth, **tight)
        assert np.allclose(nr, n, rtol=0, atol=1e-15)
        got = reference_moving(first, pl, frames[1], p, n, leaf, on, D, A, moved)
        m0 = frames[0]
        src, dst = (slice(0, w - 3), slice(3, w)) if sign > 0 else (slice(3, w), slice(0, w - 3))
        assert np.allclose(got["M"][:, dst], m0[:, src] + (frames[1][:, dst] - m0[:, src]) / 2.0, **tight)   # one tap of weight 1: W = 1
        assert np.allclose(got["N"][:, dst], 2.0, **tight) and got["history"][:, dst].all()
        gone = slice(0, 3) if sign > 0 else slice(w - 3, w)          # what slid in from outside the frame starts again
        assert (got["N"][:, gone] == 1.0).all() and np.array_equal(got["M"][:, gone], frames[1][:, gone]) and not got["history"][:, gone].any()
        assert np.array_equal(got["p"], p) and np.array_equal(got["n"], n)   # clause 6: the current surface is stored
        # without the motion (D = identity) the same pixels read their own column: the plain restatement
        still = reference_moving(first, pl, frames[1], p, n, leaf, on, D, A, np.zeros(1, dtype=bool))
        plain = reference(first, pl, frames[1], p, n, leaf, on)
        assert all(np.array_equal(still[k], plain[k]) for k in ("M", "Q", "N", "p", "n", "leaf"))
        assert np.allclose(still["M"], m0 + (frames[1] - m0) / 2.0, **tight)
    # a leaf that did not move beside one that did: its pixels are the plain restatement's, bit for bit
    leaf2 = leaf.copy()
    leaf2[:, 5:] = 1
    shift = 3.0 * depth * pl["pw"] * pl["i"]
    m2w = np.concatenate([_translation(shift), ident])
    D, A, moved = motion(m2w, np.concatenate([_translation(-shift), ident]), np.concatenate([ident, ident]), np.concatenate([ident, ident]))
    assert moved.tolist() == [True, False]
    first2 = reference(new_state(h, w), pl, frames[0], p, n, leaf2, on)
    got = reference_moving(first2, pl, frames[1], p, n, leaf2, on, D, A, moved)
    plain = reference(first2, pl, frames[1], p, n, leaf2, on)
    assert all(np.array_equal(got[k][:, 5:], plain[k][:, 5:]) for k in ("M", "Q", "N"))
    assert (got["N"][:, 3:5] == 2.0).all() and (got["N"][:, :3] == 1.0).all()
    # a change of a non-uniform scale: history written under scale (1, 1, 1), now (2, 1, 1/2).  A = diag(2, 1, 1/2), so the normal
    # (1, 1, 1) / sqrt(3) goes back to (2, 1, 1/2) / sqrt(21 / 4); D = diag(1/2, 1, 2) takes the point back
    s = np.zeros((1, 3, 4))
    s[0, :, :3] = np.diag([2.0, 1.0, 0.5])
    si = np.zeros((1, 3, 4))
    si[0, :, :3] = np.diag([0.5, 1.0, 2.0])
    D, A, moved = motion(s, si, ident, ident)
    assert moved.all() and np.array_equal(A[0], np.diag([2.0, 1.0, 0.5])) and np.array_equal(D[0], si[0])
    pt, nm = np.array([[[4.0, -3.0, 0.25]]]), np.array([[[1.0, 1.0, 1.0]]]) / math.sqrt(3.0)
    pr, nr = taken_back(pt, nm, np.zeros((1, 1), dtype=np.int32), D, A, moved)
    assert np.array_equal(pr[0, 0], [2.0, -3.0, 0.5])
    assert np.allclose(nr[0, 0], np.array([2.0, 1.0, 0.5]) / math.sqrt(5.25), rtol=1e-15, atol=0)
    # ... and a singular A gives a non-finite normal, which fails every tap: no history
    D0, A0 = D.copy(), np.zeros((1, 3, 3))
    flat_leaf = np.zeros((h, w), dtype=np.int32)
    none = reference_moving(first, pl, frames[1], p, n, flat_leaf, on, np.concatenate([_translation((0, 0, 0))]), A0, np.ones(1, dtype=bool))
    assert not none["history"].any() and (none["N"] == 1.0).all() and D0.shape == (1, 3, 4)
    # a miss pixel is never taken back
    miss = np.full((1, 1), -1, dtype=np.int32)
    pr, nr = taken_back(pt, nm, miss, D, A, moved)
    assert np.array_equal(pr, pt) and np.array_equal(nr, nm)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
CAM = dict(o=(0.0, 1.5, -9.0), look_at=(0.0, 0.6, 0.0), up=(0.0, 1.0, 0.0), fov=50.0, aspect=16.0 / 9.0)
SPHERE_AT = np.array([-4.0, 1.0, -2.0])


def _camera():
    return ft.make_camera(CAM["o"], CAM["look_at"], CAM["up"], H.deg(CAM["fov"]), CAM["aspect"])


_TRIS = []


def _bunny_tris():
    if not _TRIS:
        with open(os.path.join(H.ROOT, "scenes", "meshes", "bunny_synth_res4.ply")) as f:
            _TRIS.append(ft.parse_ply(f.read()))
    return _TRIS[0]


def _pose(t, sphere_only=False, sphere_step=0.15):
    """The transform lists of the moving nodes at time t (in calls; fractional for a commit half-way)."""
    u = 0.0 if sphere_only else t
    return dict(sphere=[("translate", tuple(SPHERE_AT + np.array([sphere_step * t, 0.0, 0.0])))],
                cube=[("rotate", (0, 1, 0), H.deg(20.0 + 2.0 * u)), ("scale", (2.0, 0.8 + 0.04 * u, 1.0)), ("translate", (12.2, 2.75, 1.5))],
                mesh=[("scale", 8.0), ("rotate", (0, 1, 0), H.deg(180.0 + 1.5 * u)), ("translate", (-4.9 + 0.05 * u, 3.2, 0.5))],
                operand=[("scale", 0.8), ("translate", (1.9 + 0.05 * u, 1.2 + 0.03 * u, -0.5))])


def _build(ctx, pose):
    """A static ground plane, an unlit sphere under a translate, a cube under rotate + non-uniform scale, the 980-face stand-in mesh as
    `bspMesh 0` under scale + rotate + translate, a CSG subtract whose second operand moves, one directional light.  Returns the handles of the
    moving transform nodes.  (The image plane is the reference's: 160 columns of width / 89 start at the left edge of the field of view,
    so the optical axis meets the frame at column 44.5, row 79.5; the cube floats where the second tile of test_denoise.py looks, the
    mesh where the first one does.)"""
    ctx.clear()
    hd = {}
    ground = ctx.material(ctx.primitive(ft.PLANE), colour=(0.6, 0.6, 0.55))
    hd["sphere"] = ctx.transform(pose["sphere"], ctx.primitive(ft.SPHERE))
    sphere = ctx.material(hd["sphere"], colour=(0.9, 0.3, 0.2), apply_lighting=False)
    hd["cube"] = ctx.transform(pose["cube"], ctx.primitive(ft.CUBE))
    cube = ctx.material(hd["cube"], colour=(0.2, 0.5, 0.9), shineyness=8.0)
    hd["mesh"] = ctx.transform(pose["mesh"], ctx.bsp_mesh(0, _bunny_tris()))
    mesh = ctx.material(hd["mesh"], colour=(0.8, 0.8, 0.3))
    hd["operand"] = ctx.transform(pose["operand"], ctx.primitive(ft.SPHERE))
    block = ctx.transform([("scale", 1.4), ("translate", (1.8, 0.7, 0.0))], ctx.primitive(ft.CUBE))
    csg = ctx.material(ctx.subtract(block, hd["operand"]), colour=(0.3, 0.8, 0.4))
    ctx.set_objects(ctx.group([ground, sphere, cube, mesh, csg]))
    ctx.add_directional((0.4, -1.0, 0.6), (1.0, 1.0, 1.0))
    ctx.commit()
    return hd


def _move(ctx, hd, pose):
    for name, ops in pose.items():
        ctx.set_transform(hd[name], ops)
    ctx.commit_moved()


def _matrices(ctx):
    m2w, w2m = ctx.leaf_matrices()
    return m2w.copy(), w2m.copy()


def _step(ctx, st, pose_of_set, cam, spp, jit, sample, seed, inside, tiles=None, follow=True):
    """render, the surfaces, accumulate, and the restatement's state after it.  pose_of_set: the (m2w, w2m) the history was written in
    (None before the first call).  follow=False: the restatement with every D forced to identity."""
    c, _ = ctx.render(cam, W, Hh, spp, jit, seed=seed)
    p, n, leaf = _surfaces(ctx, cam, W, Hh, spp, jit, sample, seed, tiles=tiles)
    out, stats = ctx.temporal_accumulate(cam, spp, jit, sample=sample, seed=seed, out=np.full((Hh, W, 3), 7.0))
    now = _matrices(ctx)
    D, A, moved = motion(now[0], now[1], *(pose_of_set or now))
    if not follow:
        moved = np.zeros_like(moved)
    st = reference_moving(st, image_plane(cam, W, Hh), c, p, n, leaf, inside, D, A, moved)
    return st, now, dict(c=c, p=p, n=n, leaf=leaf, out=out, stats=stats, moved=moved)


# ---------------------------------------------------------------------------------------------------------------- 1. device against restatement
@pytest.mark.gpu
@pytest.mark.parametrize("twice", [False, True], ids=["one-commit", "two-commits"])
@pytest.mark.parametrize("tiles", [None, TILES], ids=["frame", "tiles"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("path", ["static", "orbit"])
def test_device_matches_the_restatement(hip, path, spp, tiles, twice):
    hd = _build(hip, _pose(0.0))
    cams = orbit(_camera(), CALLS) if path == "orbit" else [_camera()] * CALLS
    jit, sample = ft.jitter_pattern(spp), spp - 1
    inside = _mask(tiles)
    hip.temporal_begin(W, Hh, tiles=tiles)
    st, pose_of_set = new_state(Hh, W), None
    n_leaves = hip.scene_info()["leaves"]
    worst, share, with_history, moved_px = 0.0, 0.0, [], []
    for k, cam in enumerate(cams):
        if k > 0:
            if twice:
                _move(hip, hd, _pose(k - 0.5))                       # a pose no accumulate ever sees
            _move(hip, hd, _pose(float(k)))
        st, pose_of_set, io = _step(hip, st, pose_of_set, cam, spp, jit, sample, 100 + k, inside, tiles=tiles)
        assert io["moved"].shape == (n_leaves,) and int(io["moved"].sum()) == (0 if k == 0 else 4)   # the sphere, the cube, the mesh, the CSG's second operand
        left_out = int(st["taint"].sum())
        share = max(share, left_out / int(inside.sum()))
        err, M, _, _ = _compare(hip, st, inside & ~st["taint"], f"motion {path} x{spp} call {k}")
        worst = max(worst, err)
        assert np.array_equal(io["out"][inside], M[inside]) and (io["out"][~inside] == 7.0).all()
        status = hip.temporal_status()
        assert status["calls"] == k + 1 and abs(status["with_history"] - int(st["history"].sum())) <= left_out
        with_history.append(status["with_history"])
        moved_px.append(int((inside & (io["leaf"] >= 0) & io["moved"][np.clip(io["leaf"], 0, None)] & st["history"]).sum()))
    print(f"temporal motion parity {path} x{spp} {'tiles' if tiles else 'frame'} {'two commits' if twice else 'one commit'} per call: worst error {worst:.3e} x the bound, "
          f"left out {share:.5%} of the tile pixels, pixels with history per call {with_history}, of them on moved leaves {moved_px}")
    assert share <= LEFT_OUT_CAP, f"{share:.5%} of the tile pixels lie within 1e-9 of a threshold"
    assert with_history[0] == 0 and min(with_history[1:]) > 0 and min(moved_px[1:]) > 0   # history was found on moved surfaces
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 2. static surfaces
def _grown(mask, r):
    out = mask.copy()
    h, w = mask.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out[max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)] |= mask[max(0, -dy):h + min(0, -dy), max(0, -dx):w + min(0, -dx)]
    return out


@pytest.mark.gpu
def test_static_surfaces_are_untouched(hip):
    """Only the sphere moves, the camera stands.  A pixel whose own leaf and whose tap leaves are static (with a static camera the taps
    lie in the pixel's 3x3 neighbourhood of the previous set) must not notice: the restatement with the motion gives, bit for bit, what
    the plain restatement of test_temporal.py gives there, and the device agrees with that within the bounds of test_temporal.py.  Then,
    device against device: a commit_moved that changes no transform leaves M, Q and N bit-identical."""
    hd = _build(hip, _pose(0.0))
    cam, jit = _camera(), np.zeros((1, 2))
    everywhere = _mask(None)
    hip.temporal_begin(W, Hh)
    st, pose_of_set, sphere_leaf = new_state(Hh, W), None, -2
    checked = 0
    for k in range(4):
        if k > 0:
            _move(hip, hd, _pose(float(k), sphere_only=True, sphere_step=0.6))
        before = st
        st, pose_of_set, io = _step(hip, st, pose_of_set, cam, 1, jit, 0, 200 + k, everywhere)
        if k == 0:
            sphere_leaf = int(np.argmin(np.abs(pose_of_set[0][:, :, 3] - SPHERE_AT).sum(-1)))
        assert np.flatnonzero(io["moved"]).tolist() == ([] if k == 0 else [sphere_leaf]) and (io["leaf"] == sphere_leaf).any()
        plain = reference(before, image_plane(cam, W, Hh), io["c"], io["p"], io["n"], io["leaf"], everywhere)
        static = (io["leaf"] != sphere_leaf) & ~_grown(before["leaf"] == sphere_leaf, 1)
        assert all(np.array_equal(st[name][static], plain[name][static], equal_nan=True) for name in ("M", "Q", "N"))
        if k > 0:
            assert not all(np.array_equal(st[name], plain[name], equal_nan=True) for name in ("M", "N"))   # the motion does matter elsewhere
        _compare(hip, plain, static & ~plain["taint"] & ~st["taint"], f"static surfaces call {k}")
        checked += int(static.sum())
    assert checked > 3 * W * Hh // 2
    # a commit_moved with nothing changed, against the same calls without it
    runs = []
    for with_commit in (False, True):
        hip.temporal_begin(W, Hh)
        for k in range(4):
            if with_commit and k > 0:
                hip.commit_moved()
            hip.render(cam, W, Hh, 1, jit, seed=300 + k, fetch=False)
            hip.temporal_accumulate(cam, 1, jit, seed=300 + k, fetch=False)
        runs.append(hip.temporal_fetch() + (hip.temporal_status(),))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0][:3], runs[1][:3])) and runs[0][3] == runs[1][3]
    assert runs[0][3]["with_history"] > 0
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 3. it follows the object
@pytest.mark.gpu
def test_history_follows_the_sphere(hip):
    """The unlit sphere slides 8 pixel widths per call, twice the default position tolerance of 4, under a static camera.  Two pixels
    inside its silhouette the history length is the number of calls; the same restatement with the motion left out finds no history."""
    cam, jit = _camera(), np.zeros((1, 2))
    pl = image_plane(cam, W, Hh)
    assert abs(pl["i"][1]) < 1e-15 and abs(pl["i"][2]) < 1e-15      # the image's x axis is the world's: a slide along x keeps the depth
    step = 8.0 * pl["pw"] * float(np.dot(SPHERE_AT - pl["o"], pl["k"])) / abs(pl["i"][0])
    hd = _build(hip, _pose(0.0))
    everywhere = _mask(None)
    hip.temporal_begin(W, Hh)
    st, lost, pose_of_set = new_state(Hh, W), new_state(Hh, W), None
    sphere_leaf = None
    for k in range(CALLS):
        if k > 0:
            _move(hip, hd, _pose(float(k), sphere_only=True, sphere_step=step))
        before = pose_of_set
        st, pose_of_set, io = _step(hip, st, before, cam, 1, jit, 0, 400 + k, everywhere)
        D, A, moved = motion(*pose_of_set, *(before or pose_of_set))
        lost = reference_moving(lost, pl, io["c"], io["p"], io["n"], io["leaf"], everywhere, D, A, np.zeros_like(moved))
        if sphere_leaf is None:
            sphere_leaf = int(np.argmin(np.abs(pose_of_set[0][:, :, 3] - SPHERE_AT).sum(-1)))
        inner = ~_grown(io["leaf"] != sphere_leaf, 2)
        M, _, N = hip.temporal_fetch()
        status = hip.temporal_status()
        print(f"temporal motion follow call {k + 1}: {int(inner.sum())} pixels two inside the sphere, N there {float(N[inner].min())} .. {float(N[inner].max())}, "
              f"without the motion {float(lost['N'][inner].min())} .. {float(lost['N'][inner].max())}, {status['with_history']} pixels with history")
        assert inner.sum() > 100
        assert (np.abs(N[inner] - (k + 1)) <= 1e-12 * (k + 1)).all()
        assert np.allclose(M[inner], io["c"][inner], rtol=1e-12, atol=0)   # unlit: every frame shows the same colour there
        if k > 0:
            assert status["with_history"] >= int(inner.sum()) and st["history"][inner].all()
            assert (lost["N"][inner] == 1.0).all() and not lost["history"][inner].any()
    hip.temporal_end()


# ---------------------------------------------------------------------------------------------------------------- 4. lifecycle
@pytest.mark.gpu
def test_lifecycle(hip):
    hd = _build(hip, _pose(0.0))
    cam, jit = _camera(), ft.jitter_pattern(2)
    everywhere = _mask(None)
    hip.progressive_begin(cam, W, Hh)
    hip.progressive_pass(2, jit, seed=1, fetch=False)
    hip.temporal_begin(W, Hh)
    hip.render(cam, W, Hh, 2, jit, seed=1, fetch=False)
    hip.temporal_accumulate(cam, 2, jit, seed=1, fetch=False)
    _move(hip, hd, _pose(1.0))
    # the progressive accumulation ended, the temporal one did not
    assert ft.hip_lib().ft_progressive_pass(hip._ctx, 2, _capi.dptr(jit), 2, 0, None, None) == -5
    assert hip.temporal_status()["calls"] == 1
    # ft_render is a fresh context's, bit for bit
    frame, _ = hip.render(cam, W, Hh, 2, jit, seed=2)
    fresh = ft.Context(device=0)
    try:
        _build(fresh, _pose(1.0))
        assert _same_bits(hip.leaf_matrices(), fresh.leaf_matrices())
        want, _ = fresh.render(cam, W, Hh, 2, jit, seed=2)
    finally:
        fresh.close()
    assert np.array_equal(frame, want, equal_nan=True)
    # the filter: with demodulate its guide pass would show another pose than the set
    with pytest.raises(ft.FtError) as e:
        hip.temporal_filter(cam, 2, jit, seed=2, demodulate=1)
    assert e.value.status == -5 and "ft_scene_commit_moved" in str(e.value)
    old, _, _ = hip.temporal_filter(demodulate=0, iterations=1)      # ... without, it filters the set as it stands
    assert np.isfinite(old).all()
    hip.temporal_accumulate(cam, 2, jit, seed=2, fetch=False)
    assert hip.temporal_status()["calls"] == 2 and hip.temporal_status()["with_history"] > 0
    hip.temporal_filter(cam, 2, jit, seed=2, demodulate=1)           # the set has the scene's pose again
    # without demodulate: test_temporal_filter.py's restatement on the moved history, twice (the second time before the next accumulate)
    for k in (3, 4):
        kw = dict(FILTER_PARAMS, iterations=3, demodulate=0, min_history=2)
        M, se, N, n, p, hit, a = _filter_inputs(hip, cam, 2, jit, 0, 2)
        got, got_v, _ = hip.temporal_filter(out=np.full((Hh, W, 3), 7.0), variance=np.full((Hh, W), 5.0), **kw)
        want, want_v, v0 = filter_reference(M, se, N, n, p, hit, everywhere, a=a, **kw)
        _filter_compare(got, got_v, want, want_v, v0, everywhere, f"moved history, filter call {k}")
        assert not np.array_equal(got, M)
        if k == 3:
            _move(hip, hd, _pose(1.0))                               # a commit that moves nothing still counts as one
            _move(hip, hd, _pose(0.0))
            _move(hip, hd, _pose(1.0))                               # ... back where the set was written: the guide pass of _filter_inputs shows its surfaces
    # ft_scene_commit still ends the temporal accumulation
    hip.commit()
    hip.render(cam, W, Hh, 2, jit, seed=3, fetch=False)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_accumulate(cam, 2, jit, seed=3)
    assert e.value.status == -5 and "ft_temporal_begin" in str(e.value)
    with pytest.raises(ft.FtError) as e:
        hip.temporal_status()
    assert e.value.status == -5
    # ... and a temporal accumulation begun after moves starts from the pose it finds
    _move(hip, hd, _pose(2.0))
    hip.temporal_begin(W, Hh)
    st, pose_of_set = new_state(Hh, W), None
    for k in range(2):
        if k:
            _move(hip, hd, _pose(3.0))
        st, pose_of_set, io = _step(hip, st, pose_of_set, cam, 2, jit, 0, 500 + k, everywhere)
        _compare(hip, st, everywhere & ~st["taint"], f"begun after moves, call {k}")
    assert hip.temporal_status()["with_history"] > 0
    hip.temporal_end()

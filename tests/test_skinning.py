"""Skinning (ft_sg_set_mesh_skin / ft_sg_set_mesh_bones / ft_debug_skin): per corner J bone indices and weights, a palette
of 3x4 bone matrices per pose, the vertices posed by k_skin into the buffer the refit reads (ft_skin.hip) and scanned there by the morph
kernels.

The promise under test: set_mesh_bones(node, P) followed by any commit gives every bit that set_mesh_triangles(node, V) gives on a twin
node without a skin, V = functracer_amd.skin_blend(shape, index, weight, P) - the formula of the header in numpy, one elementwise IEEE
operation per step.  Every comparison is bitwise; there is no tolerance in this file."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import bvh_tools as B
from . import helpers as H
from .test_light_space_shadows import light_space
from .test_mesh_refit import CAT, RES, SPP, Recorder, _ground_scene, answers, assert_same_answers, assert_same_topology, contexts, deform, same  # noqa: F401 (contexts: a fixture)
from .test_morph_targets import TREE_KEYS, _zero_mesh, replay_scan, same_trees, targets_of, view_of

LABELS = ("one-hot", "equal", "mixed", "tiny", "cancel")


def palette(n_bones, seed, centre=(0.0, 0.0, 0.0), radius=1.0, amount=1.0):
    """n_bones 3x4 matrices from a seeded generator: a rotation about an arbitrary axis times a non-uniform scale, about `centre`, plus a
    translation of a fraction of `radius`.  [n_bones, 12]."""
    rng = np.random.default_rng(seed)
    centre = np.asarray(centre, dtype=np.float64)
    out = np.zeros((n_bones, 3, 4))
    for b in range(n_bones):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = amount * rng.uniform(-0.6, 0.6)
        K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        R = np.eye(3) + math.sin(ang) * K + (1.0 - math.cos(ang)) * (K @ K)
        A = R @ np.diag(rng.uniform(0.8, 1.25, size=3))
        out[b, :, :3] = A
        out[b, :, 3] = centre - A @ centre + amount * rng.uniform(-0.2, 0.2, size=3) * radius
    return out.reshape(n_bones, 12)


def skin_of(n_tris, J, n_bones, label, seed=3):
    """Indices and weights [n_tris, 3, J] of weight set `label`: one-hot, equal shares, mixed signs that do not sum to 1, shares of 1e-300
    beside a 1, and (J = 4) a set whose partial sums cancel - slots 0 and 2 name the same bone, so the order of the terms shows."""
    rng = np.random.default_rng(seed)
    index = rng.integers(0, n_bones, size=(n_tris, 3, J)).astype(np.int32)
    index.reshape(-1)[-1] = n_bones - 1                              # the palette's last bone is used
    sets = {"one-hot": [1.0, 0.0, 0.0, 0.0], "equal": [1.0 / J] * 4, "mixed": [0.7, -0.4, 0.9, 0.15], "tiny": [1.0, 1e-300, 1e-300, 1e-300], "cancel": [1e16, 1.0, -1e16, 0.5]}
    weight = np.broadcast_to(np.array(sets[label][:J]), (n_tris, 3, J)).copy()
    if label == "cancel":
        assert J == 4
        index[:, :, 2] = index[:, :, 0]
    return index, weight


def pose_of(e, J, n_bones, label, seed=3, amount=1.0):
    base = e.tris.reshape(-1, 9)
    index, weight = skin_of(base.shape[0], J, n_bones, label, seed)
    return base, index, weight, palette(n_bones, seed + 100, e.centre, e.radius, amount)


def skin_bytes(base, J, n_bones, rest=True):
    corners = base.shape[0] * 3
    return (base.size * 8 if rest else 0) + corners * 4 + corners * J * 8 + n_bones * 96


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_bindings_declare_the_skin_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert "#define FT_MAX_SKIN_BONES 256" in hdr and "#define FT_MAX_SKIN_INFLUENCES 4" in hdr and "#define FT_ABI_VERSION 2" in hdr and '"skin_on_device"' in hdr
    assert "stays welded" in hdr
    assert re.search(r"int32_t ft_sg_set_mesh_skin\(ft_context\* ctx, ft_node mesh, const int32_t\* bone_index, const double\* bone_weight, int32_t influences, int64_t n_tris\);", hdr)
    assert re.search(r"int32_t ft_sg_set_mesh_bones\(ft_context\* ctx, ft_node mesh, const double\* matrices, int32_t n_bones\);", hdr)
    assert re.search(r"int32_t ft_debug_skin\(ft_context\* ctx, ft_node mesh, int64_t counts\[4\]\);", hdr)
    lib = C.CDLL(ft.HIP_LIB)
    doc = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    for name in ("ft_sg_set_mesh_skin", "ft_sg_set_mesh_bones", "ft_debug_skin"):
        assert hasattr(lib, name), name
        assert re.search(r"\[<DllImport\(Lib\)>\] extern int " + name + r"\(", doc), name
        assert name in [s[0] for s in _capi.SKIN_SIGNATURES]
    for name in ("set_mesh_skin", "set_mesh_bones", "skin"):
        assert callable(getattr(ft.Context, name)), name
    assert callable(ft.skin_blend) and _capi.MAX_SKIN_BONES == 256 and _capi.MAX_SKIN_INFLUENCES == 4
    ctx = ft.Context(host_only=True)
    for v in (0, 1, 7, -1):
        ctx.set_option("skin_on_device", v)
    ctx.close()


def _small(ctx):
    ctx.clear()
    hd = {"flat": ctx.bsp_mesh(0, CAT["blob(9)"].tris.reshape(-1, 9))}
    hd["xf"] = ctx.transform([("translate", (3, 0, 0))], ctx.primitive(ft.CUBE))
    ctx.set_objects(ctx.group([hd["flat"], hd["xf"]]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    return hd


def test_the_setters_refuse_bad_arguments_and_change_nothing():
    ctx = ft.Context(host_only=True)
    hd = _small(ctx)
    lib = ft.hip_lib()
    T0, info0 = ctx.mesh_trees(), ctx.scene_info()
    e = CAT["blob(9)"]
    _, index, weight, bones = pose_of(e, 2, 3, "mixed")
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    pi, pw, pb = ip(index), _capi.dptr(weight), _capi.dptr(bones)
    skin = lambda *a: lib.ft_sg_set_mesh_skin(*a)                    # noqa: E731
    set_bones = lambda *a: lib.ft_sg_set_mesh_bones(*a)                  # noqa: E731
    assert set_bones(ctx._ctx, hd["flat"], pb, 3) == -1                 # bones without a skin
    assert skin(None, hd["flat"], pi, pw, 2, 9) == -1
    assert skin(ctx._ctx, -1, pi, pw, 2, 9) == -1 and skin(ctx._ctx, 10_000, pi, pw, 2, 9) == -1
    assert skin(ctx._ctx, hd["xf"], pi, pw, 2, 9) == -1             # a transform node
    for n in (8, 10, 0, -1):
        assert skin(ctx._ctx, hd["flat"], pi, pw, 2, n) == -1, n
    for j in (-1, 5):
        assert skin(ctx._ctx, hd["flat"], pi, pw, j, 9) == -1, j
    assert skin(ctx._ctx, hd["flat"], None, pw, 2, 9) == -1 and skin(ctx._ctx, hd["flat"], pi, None, 2, 9) == -1
    for bad in (-1, 256, 1 << 20):
        ib = index.copy()
        ib[4, 1, 1] = bad
        assert skin(ctx._ctx, hd["flat"], ip(ib), pw, 2, 9) == -1, bad
    for bad in (np.nan, np.inf, -np.inf):
        wb = weight.copy()
        wb[8, 2, 1] = bad
        assert skin(ctx._ctx, hd["flat"], pi, _capi.dptr(wb), 2, 9) == -1, bad
    assert set_bones(ctx._ctx, hd["flat"], pb, 3) == -1                 # every call above was refused: still no skin
    assert skin(ctx._ctx, hd["flat"], pi, pw, 2, 9) == 0
    assert set_bones(None, hd["flat"], pb, 3) == -1 and set_bones(ctx._ctx, hd["xf"], pb, 3) == -1 and set_bones(ctx._ctx, -1, pb, 3) == -1
    assert set_bones(ctx._ctx, hd["flat"], None, 3) == -1
    big = np.ascontiguousarray(np.resize(bones, (257, 12)))
    for n in (-1, 257):
        assert set_bones(ctx._ctx, hd["flat"], _capi.dptr(big), n) == -1, n
    for n in (1, 2):                                                 # the skin uses bone 2
        assert set_bones(ctx._ctx, hd["flat"], pb, n) == -1, n
    for bad in (np.nan, np.inf, -np.inf):
        bb = bones.copy()
        bb[1, 7] = bad
        assert set_bones(ctx._ctx, hd["flat"], _capi.dptr(bb), 3) == -1, bad
    counts = (C.c_int64 * 4)()
    assert lib.ft_debug_skin(ctx._ctx, hd["xf"], counts) == -1 and lib.ft_debug_skin(None, hd["flat"], counts) == -1 and lib.ft_debug_skin(ctx._ctx, hd["flat"], None) == -1
    ctx.commit_deformed()                                            # nothing was marked: the commit of before, bit for bit
    same_trees(ctx.mesh_trees(), T0, "after the refused calls")
    ctx.commit()
    same_trees(ctx.mesh_trees(), T0, "after the refused calls and a full commit")
    assert ctx.scene_info() == info0
    assert skin(ctx._ctx, hd["flat"], None, None, 0, 9) == 0        # removes it
    assert set_bones(ctx._ctx, hd["flat"], pb, 3) == -1
    ctx.close()


def _rounded(x):
    return Fraction(float(x))


def _exact(shape, index, weight, bones):
    """The header's formula in exact rational arithmetic, every product and sum rounded to double once."""
    p = shape.reshape(-1, 3)
    idx, w, M = index.reshape(p.shape[0], -1), weight.reshape(p.shape[0], -1), bones.reshape(-1, 3, 4)
    out = np.zeros_like(p)
    for c in range(p.shape[0]):
        x, y, z = (Fraction(float(v)) for v in p[c])
        for i in range(3):
            acc = None
            for j in range(idx.shape[1]):
                m = [Fraction(float(v)) for v in M[idx[c, j], i]]
                t = _rounded(_rounded(m[0] * x) + _rounded(m[1] * y))
                t = _rounded(t + _rounded(m[2] * z))
                t = _rounded(t + m[3])
                q = _rounded(Fraction(float(w[c, j])) * t)
                acc = q if j == 0 else _rounded(acc + q)
            out[c, i] = float(acc)
    return out.reshape(-1, 9)


def _fma(a, b, c):
    return math.fma(a, b, c) if hasattr(math, "fma") else float(Fraction(a) * Fraction(b) + Fraction(c))


def _fused(shape, index, weight, bones):
    """skin_blend() with every multiply-add fused - what the library must NOT compute."""
    p = shape.reshape(-1, 3)
    idx, w, M = index.reshape(p.shape[0], -1), weight.reshape(p.shape[0], -1), bones.reshape(-1, 3, 4)
    out = np.zeros_like(p)
    for c in range(p.shape[0]):
        x, y, z = (float(v) for v in p[c])
        for i in range(3):
            acc = 0.0
            for j in range(idx.shape[1]):
                m = [float(v) for v in M[idx[c, j], i]]
                t = _fma(m[2], z, _fma(m[1], y, m[0] * x)) + m[3]
                acc = float(w[c, j]) * t if j == 0 else _fma(float(w[c, j]), t, acc)
            out[c, i] = acc
    return out.reshape(-1, 9)


@pytest.mark.parametrize("label", LABELS)
def test_skin_blend_is_the_formula_rounded_once_per_step(label):
    e = CAT["blob(9)"]
    J = 4
    base, index, weight, bones = pose_of(e, J, 5, label)
    base = np.concatenate([base, deform(e, "far")[0].reshape(-1, 9)])[:17]   # 51 corners, near and far from the origin
    index, weight = skin_of(17, J, 5, label)
    got = ft.skin_blend(base, index, weight, bones)
    assert got.shape == (17, 9) and np.array_equal(got, _exact(base, index, weight, bones)), label
    for j in (1, 2, 3):                                              # fewer influences: the first j slots
        assert np.array_equal(ft.skin_blend(base, index[:, :, :j], weight[:, :, :j], bones), _exact(base, index[:, :, :j], weight[:, :, :j], bones)), (label, j)


def test_a_fused_step_would_change_the_chosen_inputs():
    base, index, weight, bones = pose_of(CAT["blob(9)"], 4, 5, "mixed")
    assert (_fused(base, index, weight, bones) != ft.skin_blend(base, index, weight, bones)).any(), "the never-fused case is vacuous: fusing changes no bit of it"
    base, index, weight, bones = pose_of(CAT["blob(9)"], 1, 3, "one-hot")
    assert (_fused(base, index, weight, bones) != ft.skin_blend(base, index, weight, bones)).any(), "J = 1: fusing the matrix rows changes no bit"


def _moved_scene(b, tris, shift):
    b.clear()
    m = b.bsp_mesh(0, tris.reshape(-1, 9))
    xf = b.transform([("translate", (shift, 0, 0))], m)
    b.set_objects(b.group([xf]))
    b.add_directional((1, -2, 1), (1, 1, 1))
    b.commit()
    return m, xf


@pytest.mark.parametrize("J", [1, 4])
@pytest.mark.parametrize("name", ["blob(9)", "degenerate", "identical"])
def test_host_only_bones_give_the_bits_of_explicit_vertices(name, J):
    e = CAT[name]
    ctx, twin, fresh = ft.Context(host_only=True), ft.Context(host_only=True), ft.Context(host_only=True)
    for label in LABELS:
        if (label == "cancel" and J != 4) or (label == "tiny" and J == 1):
            continue
        base, index, weight, bones = pose_of(e, J, 7, label)
        v = ft.skin_blend(base, index, weight, bones)
        for commit in ("commit", "commit_moved", "commit_deformed"):
            what = f"{name}, J = {J}, {label}, {commit}"
            (m, xf), (m2, xf2) = _moved_scene(ctx, base, 0.0), _moved_scene(twin, base, 0.0)
            ctx.set_mesh_skin(m, index, weight)
            ctx.set_mesh_bones(m, bones)
            twin.set_mesh_triangles(m2, v)
            shift = 0.0
            if commit == "commit_moved":                             # with a pose pending: the full commit
                shift = 1.5
                ctx.set_transform(xf, [("translate", (shift, 0, 0))])
                twin.set_transform(xf2, [("translate", (shift, 0, 0))])
            getattr(ctx, commit)()
            getattr(twin, commit)()
            _moved_scene(fresh, v, shift)
            got = ctx.mesh_trees()
            same_trees(got, twin.mesh_trees(), what + " (set_mesh_triangles)")
            same_trees(got, fresh.mesh_trees(), what + " (fresh graph)")
            assert all(same(x, y) for x, y in zip(ctx.leaf_matrices(), fresh.leaf_matrices())), what
            if commit == "commit_deformed":
                s, mo = ctx.skin(m), ctx.morph(m)
                assert (s["device_commits"], s["device_meshes"], s["host_meshes"], s["resident_bytes"]) == (0, 0, 1, 0), what
                assert not mo["from_device"] and same(mo["scan"][:7], replay_scan(v)), what
    for c in (ctx, twin, fresh):
        c.close()


def test_the_order_rules_of_the_setters():
    e = CAT["blob(65)"]
    base, index, weight, bones = pose_of(e, 4, 6, "mixed")
    targets = targets_of(e, 3)
    ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)

    def expect(tris, what):
        _moved_scene(fresh, tris, 0.0)
        same_trees(ctx.mesh_trees(), fresh.mesh_trees(), what)
    m, _ = _moved_scene(ctx, base, 0.0)
    ctx.set_mesh_skin(m, index, weight)
    ctx.commit_deformed()                                            # a skin alone is no edit
    expect(base, "set_mesh_skin alone changes no vertex")
    ctx.set_mesh_bones(m, bones)
    ctx.commit_deformed()
    expect(ft.skin_blend(base, index, weight, bones), "bones")
    shape2 = deform(e, "twist", 0.3)[0].reshape(-1, 9)
    ctx.set_mesh_triangles(m, shape2)                                # a new U under the palette in force
    ctx.commit_deformed()
    expect(ft.skin_blend(shape2, index, weight, bones), "set_mesh_triangles under a palette re-poses the new shape")
    ctx.set_mesh_targets(m, targets)                                 # the base is U (shape2), not the skinned V; no edit
    ctx.commit_deformed()
    expect(ft.skin_blend(shape2, index, weight, bones), "set_mesh_targets under a palette changes no vertex")
    w = [0.3, -0.2, 0.5]
    ctx.set_mesh_weights(m, w)
    ctx.commit_deformed()
    blended = ft.morph_blend(shape2, targets, w)
    expect(ft.skin_blend(blended, index, weight, bones), "set_mesh_weights under a palette gives skin(blend), the base being the shape")
    bones2 = palette(6, 77, e.centre, e.radius)
    ctx.set_mesh_bones(m, bones2)
    ctx.commit()                                                     # a full commit skins on demand
    expect(ft.skin_blend(blended, index, weight, bones2), "a new palette over the blended shape, full commit")
    ctx.set_mesh_bones(m, np.zeros((0, 12)))                         # n_bones = 0: V is U again, and that is an edit
    ctx.commit_deformed()
    expect(blended, "n_bones = 0 restores the shape")
    ctx.set_mesh_bones(m, bones)
    ctx.commit_deformed()
    expect(ft.skin_blend(blended, index, weight, bones), "the skin stayed")
    ctx.set_mesh_skin(m, np.zeros((base.shape[0], 3, 0), dtype=np.int32), np.zeros((base.shape[0], 3, 0)))   # influences = 0 under a palette: an edit
    ctx.commit_deformed()
    expect(blended, "influences = 0 restores the shape")
    assert ctx._lib.ft_sg_set_mesh_bones(ctx._ctx, m, _capi.dptr(bones), 6) == -1, "the skin is gone"
    ctx.set_mesh_skin(m, index, weight)
    ctx.set_mesh_bones(m, bones)
    ctx.set_mesh_skin(m, index[:, :, :2], weight[:, :, :2])          # a new skin removes the palette
    ctx.commit_deformed()
    expect(blended, "set_mesh_skin removes the palette")
    ctx.close(), fresh.close()


def test_a_mesh_welded_in_its_rest_pose_stays_welded():
    rng = np.random.default_rng(12)
    points = rng.normal(size=(40, 3))
    pidx, pw = rng.integers(0, 9, size=(40, 4)).astype(np.int32), rng.uniform(-0.5, 1.0, size=(40, 4))
    faces = rng.integers(0, 40, size=(120, 3))                       # every point is the corner of several triangles
    base, index, weight = points[faces].reshape(-1, 9), pidx[faces], pw[faces]
    bones = palette(9, 8)
    v = ft.skin_blend(base, index, weight, bones).reshape(-1, 3)
    flat = faces.reshape(-1)
    for p in range(40):
        rows = v[flat == p]
        assert len(rows) and all(same(r, rows[0]) for r in rows), p
    ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)
    m, _ = _moved_scene(ctx, base, 0.0)
    ctx.set_mesh_skin(m, index, weight)
    ctx.set_mesh_bones(m, bones)
    ctx.commit_deformed()
    _moved_scene(fresh, v.reshape(-1, 9), 0.0)
    same_trees(ctx.mesh_trees(), fresh.mesh_trees(), "welded")
    ctx.close(), fresh.close()


def test_a_palette_that_overflows_is_refused_and_the_old_commit_stays():
    ctx = ft.Context(host_only=True)
    e = CAT["blob(9)"]
    base, index, weight, bones = pose_of(e, 2, 3, "equal")
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    T0 = ctx.mesh_trees()
    ctx.set_mesh_skin(rec.meshes[0], index, weight)
    ctx.set_mesh_bones(rec.meshes[0], np.full((3, 12), 1e300))
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    same_trees(ctx.mesh_trees(), T0, "after the refused commit")
    ctx.set_mesh_bones(rec.meshes[0], bones)
    ctx.commit_deformed()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _options(*ctxs, **opts):
    base = {"bvh_builder": 2, "primary_block_lists": 1, "light_space_shadows": 2, "deform_light_space": 0, "light_space_retree": 0, "refit_rebuild_percent": 0,
            "temporal_follow_deformed": 0, "morph_on_device": 1, "skin_on_device": 1}
    base.update(opts)
    for c in ctxs:
        for k, v in base.items():
            c.set_option(k, v)


# each mesh, J and bone count with each builder, each weight set with each builder
CASES = [(0, "blob(7)", 1, 3, "one-hot"), (0, "blob(65)", 2, 256, "equal"), (0, "blob(257)", 4, 3, "cancel"), (0, "blob(1025)", 4, 256, "mixed"),
         (0, "degenerate", 2, 1, "tiny"), (0, "flat", 1, 256, "mixed"), (0, "identical", 4, 1, "equal"),
         (3, "blob(7)", 4, 256, "cancel"), (3, "blob(65)", 1, 1, "one-hot"), (3, "blob(257)", 2, 3, "tiny"), (3, "blob(1025)", 2, 256, "mixed"),
         (3, "degenerate", 4, 3, "equal"), (3, "flat", 2, 1, "one-hot"), (3, "identical", 1, 3, "mixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("builder,name,J,n_bones,label", CASES)
def test_bones_give_every_bit_that_explicit_vertices_give(contexts, builder, name, J, n_bones, label):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, bvh_builder=builder)
    e = CAT[name]
    what = f"builder {builder}, {name}, J = {J}, {n_bones} bones, {label}"
    base, index, weight, bones = pose_of(e, J, n_bones, label)
    v = ft.skin_blend(base, index, weight, bones)
    view = view_of(v)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    node = rec.meshes[0]
    T0 = ctx.mesh_trees()
    commits = ctx.skin(node)["device_commits"]
    ctx.set_mesh_skin(node, index, weight)
    ctx.set_mesh_bones(node, bones)
    ctx.commit_deformed()
    s, m = ctx.skin(node), ctx.morph(node)
    assert (s["device_commits"], s["device_meshes"], s["host_meshes"]) == (commits + 1, 1, 0), what
    assert s["resident_bytes"] == skin_bytes(base, J, n_bones), what
    assert (m["device_meshes"], m["host_meshes"], m["from_device"]) == (0, 0, True), what
    assert same(m["scan"][:7], replay_scan(v)), f"{what}: the device scan is not scan_mesh's"
    got, T1 = answers(ctx, view, v.reshape(-1, 3, 3)), ctx.mesh_trees()
    if label != "cancel":
        assert got["hit"].any() and (got["frame"] != got["frame"][0, 0]).any(), f"{what}: the mesh is not in the view"
    assert_same_topology(T0, T1, what)
    twin.set_mesh_triangles(rec2.meshes[0], v)                       # the twin node without a skin
    twin.commit_deformed()
    assert_same_answers(got, answers(twin, view, v.reshape(-1, 3, 3)), what + " (twin)")
    same_trees(T1, twin.mesh_trees(), what + " (twin)")
    ctx.set_option("skin_on_device", 0)                              # the host route: the same bits
    ctx.set_mesh_bones(node, bones)
    ctx.commit_deformed()
    s, m = ctx.skin(node), ctx.morph(node)
    assert (s["device_commits"], s["device_meshes"], s["host_meshes"], m["from_device"]) == (commits + 1, 0, 1, False), what
    assert same(m["scan"][:7], replay_scan(v)), what
    same_trees(ctx.mesh_trees(), T1, what + " (skin_on_device 0)")
    assert same(ctx.render(B.camera(*view), RES, RES, SPP, ft.jitter_pattern(SPP))[0], got["frame"]), what + " (skin_on_device 0)"
    ctx.set_option("skin_on_device", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["bone-255-everywhere", "bone-255-and-0", "one-bone-of-many"])
def test_the_last_bone_of_a_full_palette_and_one_bone_for_every_corner(contexts, case):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin)
    e = CAT["blob(257)"]
    base, index, weight, bones = pose_of(e, 2, 256, "equal")
    if case == "bone-255-everywhere":
        index[:] = 255
    elif case == "bone-255-and-0":
        index[:, :, 0], index[:, :, 1] = 255, 0
    else:
        index[:] = 17                                                # every lane reads the same matrix
    v = ft.skin_blend(base, index, weight, bones)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    ctx.set_mesh_skin(rec.meshes[0], index, weight)
    ctx.set_mesh_bones(rec.meshes[0], bones)
    ctx.commit_deformed()
    assert ctx.skin(rec.meshes[0])["device_meshes"] == 1 and same(ctx.morph(rec.meshes[0])["scan"][:7], replay_scan(v))
    twin.set_mesh_triangles(rec2.meshes[0], v)
    twin.commit_deformed()
    same_trees(ctx.mesh_trees(), twin.mesh_trees(), case)
    cam, jit = B.camera(*view_of(v)), ft.jitter_pattern(SPP)
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0]), case


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["device", "morph_on_device 0", "skin_on_device 0"])
def test_morph_then_skin_in_one_commit(contexts, route):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, morph_on_device=0 if route == "morph_on_device 0" else 1, skin_on_device=0 if route == "skin_on_device 0" else 1)
    e = CAT["blob(1025)"]
    base, index, weight, bones = pose_of(e, 4, 12, "mixed")
    targets = targets_of(e, 3)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    node = rec.meshes[0]
    ctx.set_mesh_targets(node, targets)
    ctx.set_mesh_skin(node, index, weight)
    for w, seed in (([0.3, -0.2, 0.5], 1), ([0.1, 0.6, 0.0], 2)):
        pal = palette(12, 200 + seed, e.centre, e.radius)
        v = ft.skin_blend(ft.morph_blend(base, targets, w), index, weight, pal)
        ctx.set_mesh_weights(node, w)
        ctx.set_mesh_bones(node, pal)
        ctx.commit_deformed()
        s, m = ctx.skin(node), ctx.morph(node)
        if route == "device":
            assert (s["device_meshes"], s["host_meshes"], m["device_meshes"], m["host_meshes"], m["from_device"]) == (1, 0, 1, 0, True)
            assert s["resident_bytes"] == skin_bytes(base, 4, 12, rest=False), "the shape comes from the blend: no rest shape is resident"
        else:                                                        # the host route by rule: V is made by GraphNode::vertices
            assert (s["device_meshes"], s["host_meshes"], m["device_meshes"], m["host_meshes"], m["from_device"]) == (0, 1, 0, 1, False)
        assert same(m["scan"][:7], replay_scan(v)), route
        twin.set_mesh_triangles(rec2.meshes[0], v)
        twin.commit_deformed()
        same_trees(ctx.mesh_trees(), twin.mesh_trees(), route)
        cam, jit = B.camera(*view_of(v)), ft.jitter_pattern(SPP)
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0]), route
    _options(ctx, twin)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["minus-first", "plus-first", "minus-first-across-blocks", "plus-first-across-blocks"])
def test_a_zero_bound_keeps_the_sign_of_the_first_skinned_zero(contexts, case):
    ctx = contexts("work")
    _options(ctx)
    first = -0.0 if case.startswith("minus") else 0.0
    places = (100, 500) if case.endswith("blocks") else (10, 20)
    base = _zero_mesh(first, -first, *places)                        # x >= 0, y <= 0, z > 0; the extreme x and y are zeros of both signs
    # An identity whose zero entries are signed so that every product with this mesh's coordinates is -0.0 (y < 0, z > 0, x > 0): a sum
    # of -0.0 terms keeps a -0.0 coordinate and leaves a +0.0 one as it is.
    bones = np.array([[1.0, 0.0, -0.0, -0.0, -0.0, 1.0, -0.0, -0.0, -0.0, 0.0, 1.0, -0.0]])
    index, weight = np.zeros((base.shape[0], 3, 1), dtype=np.int32), np.ones((base.shape[0], 3, 1))
    v = ft.skin_blend(base, index, weight, bones)
    zeros = v[v == 0.0]
    assert same(v, base) and np.signbit(zeros).any() and not np.signbit(zeros).all() and zeros.size >= 4
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    node = rec.meshes[0]
    ctx.set_mesh_skin(node, index, weight)
    ctx.set_mesh_bones(node, bones)
    ctx.commit_deformed()
    m, want = ctx.morph(node), replay_scan(v)
    assert ctx.skin(node)["device_meshes"] == 1 and m["from_device"] and same(m["scan"][:7], want), (m["scan"], want)
    assert m["scan"][0] == 0.0 and bool(np.signbit(m["scan"][0])) == bool(np.signbit(first)), "lower x bound: not the first zero's sign"
    assert m["scan"][4] == 0.0 and bool(np.signbit(m["scan"][4])) == bool(np.signbit(first)), "upper y bound: not the first zero's sign"
    twin = contexts("fresh")
    _options(twin)
    rec2 = Recorder(twin)
    B.build_scene(rec2, base)
    twin.set_mesh_triangles(rec2.meshes[0], v)
    twin.commit_deformed()
    assert same(twin.morph(rec2.meshes[0])["scan"][:7], m["scan"][:7])
    same_trees(ctx.mesh_trees(), twin.mesh_trees(), case)


@pytest.mark.gpu
def test_a_skinned_a_morph_and_an_explicit_mesh_in_one_commit(contexts):
    ctx, twin = contexts("work"), contexts("twin")
    _options(ctx, twin)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_multi(rec)
    B.build_multi(rec2)
    node = {part[0]: h for part, h in zip(B.MULTI_PARTS, rec.meshes)}
    cam, jit = B.camera(*B.MULTI_VIEW), ft.jitter_pattern(SPP)
    T0 = ctx.mesh_trees()
    new = {}
    base, index, weight, bones = pose_of(CAT["blob(257)"], 3, 20, "mixed")
    ctx.set_mesh_skin(node["blob(257)"], index, weight)
    ctx.set_mesh_bones(node["blob(257)"], bones)
    new["blob(257)"] = ft.skin_blend(base, index, weight, bones)
    mb, targets, w = CAT["blob(1025)"].tris.reshape(-1, 9), targets_of(CAT["blob(1025)"], 2), [0.3, 0.05]
    ctx.set_mesh_targets(node["blob(1025)"], targets)
    ctx.set_mesh_weights(node["blob(1025)"], w)
    new["blob(1025)"] = ft.morph_blend(mb, targets, w)
    new["blob(8)"] = deform(CAT["blob(8)"], "jitter")[0].reshape(-1, 9)
    ctx.set_mesh_triangles(node["blob(8)"], new["blob(8)"])
    ctx.commit_deformed()
    s, m = ctx.skin(node["blob(257)"]), ctx.morph(node["blob(8)"])
    assert (s["device_meshes"], s["host_meshes"], m["device_meshes"], m["host_meshes"], m["from_device"]) == (1, 0, 1, 0, False)
    for name in new:
        mm = ctx.morph(node[name])
        assert mm["from_device"] == (name != "blob(8)") and same(mm["scan"][:7], replay_scan(new[name])), name
    assert ctx.skin(node["blob(1025)"])["resident_bytes"] == 0 and not ctx.morph(node["blob(7)"])["scan"].any()
    T1 = ctx.mesh_trees()
    assert_same_topology(T0, T1, "multi")
    for part, h in zip(B.MULTI_PARTS, rec2.meshes):
        if part[0] in new:
            twin.set_mesh_triangles(h, new[part[0]])
    twin.commit_deformed()
    same_trees(T1, twin.mesh_trees(), "three routes against explicit vertices")
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("percent", [0, 100])
def test_six_bone_commits_in_a_row_then_a_full_commit(contexts, percent):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh, bvh_builder=3, refit_rebuild_percent=percent)
    fresh.set_option("refit_rebuild_percent", 0)
    e = CAT["blob(1025)"]
    base, index, weight, _ = pose_of(e, 4, 16, "equal")
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    node = rec.meshes[0]
    ctx.set_mesh_skin(node, index, weight)
    cam, jit = B.camera(e.centre, 2.5 * e.radius), ft.jitter_pattern(SPP)
    for step in range(1, 7):
        bones = palette(16, 300 + step, e.centre, e.radius, amount=0.4 * step)
        ctx.set_mesh_bones(node, bones)
        ctx.commit_deformed()
        assert ctx.skin(node)["device_meshes"] == 1 and ctx.morph(node)["from_device"]
        v = ft.skin_blend(base, index, weight, bones)
        B.build_scene(fresh, v)
        want = fresh.render(cam, RES, RES, SPP, jit)[0]
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], want), f"step {step}"
    B.check_trees(ctx.mesh_trees())
    ctx.commit()                                                     # the host skins the vertices it never saw
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], want)
    same_trees(ctx.mesh_trees(), fresh.mesh_trees(), "the full commit after six bone commits")
    _options(ctx, fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("retree", [0, 1])
def test_light_space_structures_follow_the_bones(contexts, retree):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, deform_light_space=1, light_space_retree=retree)
    e = CAT["blob(1025)"]
    base, index, weight, _ = pose_of(e, 2, 8, "equal")
    cam, jit = B.camera(e.centre, 2.0 * e.radius), ft.jitter_pattern(SPP)
    nodes = [_ground_scene(c, base) for c in (ctx, twin)]
    ctx.set_mesh_skin(nodes[0], index, weight)
    for seed in (1, 2):
        bones = palette(8, 400 + seed, e.centre, e.radius, amount=0.5)
        v = ft.skin_blend(base, index, weight, bones)
        ctx.set_mesh_bones(nodes[0], bones)
        ctx.commit_deformed()
        assert ctx.morph(nodes[0])["from_device"] and ctx.skin(nodes[0])["device_meshes"] == 1
        twin.set_mesh_triangles(nodes[1], v)
        twin.commit_deformed()
        got, want = light_space(ctx), light_space(twin)
        assert got[3][0] != 0xFFFFFFFF, "the caster's leaf lost its pairs"
        for a, b, what in zip(got, want, ("pairs", "nodes and grids", "records", "leaf pairs")):
            assert same(a, b), what
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])
        fresh = contexts("twin")                                     # and a fresh commit of the same vertices
        _options(fresh, deform_light_space=1, light_space_retree=retree)
        _ground_scene(fresh, v)
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], fresh.render(cam, RES, RES, SPP, jit)[0]), "a fresh commit's frame"
    _options(ctx, twin, contexts("twin"))


@pytest.mark.gpu
@pytest.mark.parametrize("follow", [0, 1])
def test_the_temporal_accumulation_follows_bones_as_it_follows_vertices(contexts, follow):
    W, Hh, calls = 96, 64, 6
    e = CAT["blob(257)"]
    base, index, weight, _ = pose_of(e, 2, 5, "equal")
    jit = np.zeros((1, 2))
    cams = [B.camera(e.centre + np.array([0.05 * k, 0.0, 0.0]), 2.0 * e.radius) for k in range(calls)]
    rest = np.tile(np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]), (5, 1))

    def run(ctx, by_bones):
        m = _ground_scene(ctx, base)
        if by_bones:
            ctx.set_mesh_skin(m, index, weight)
        ctx.temporal_begin(W, Hh)
        out = []
        for k, cam in enumerate(cams):
            if k:
                bones = rest if k < 3 else palette(5, 500, e.centre, e.radius, amount=0.3 * (k - 2))
                if by_bones:
                    ctx.set_mesh_bones(m, bones)
                else:
                    ctx.set_mesh_triangles(m, ft.skin_blend(base, index, weight, bones))
                ctx.commit_deformed()
            ctx.render(cam, W, Hh, 1, jit, seed=100 + k, fetch=False)
            ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
            out.append(([np.asarray(a).tobytes() for a in ctx.temporal_fetch()], ctx.temporal_status()))
        ctx.temporal_end()
        return out
    _options(contexts("work"), contexts("fresh"), temporal_follow_deformed=follow)
    explicit, bones = run(contexts("fresh"), False), run(contexts("work"), True)
    assert explicit == bones and bones[-1][1]["calls"] == calls
    _options(contexts("work"), contexts("fresh"))


@pytest.mark.gpu
def test_refusals_on_the_device_leave_the_old_commit(contexts):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin)
    e = CAT["blob(257)"]
    base, index, weight, bones = pose_of(e, 2, 4, "equal")
    cam, jit = B.camera(1e6 * e.centre, 3e6 * e.radius), ft.jitter_pattern(SPP)   # (the scene is the mesh a million times its size)

    def build(c, tris, depth=0):
        c.clear()
        m = c.bsp_mesh(depth, tris)
        c.set_objects(c.group([c.transform([("scale", (1e6, 1e6, 1e6))], c.material(m, colour=(0.9, 0.5, 0.2)))]))
        c.add_directional((1, -2, 1), (1, 1, 1))
        c.commit()
        return m
    m = build(ctx, base)
    ctx.set_mesh_skin(m, index, weight)
    ctx.set_mesh_bones(m, bones)
    ctx.commit_deformed()
    frame, T1 = ctx.render(cam, RES, RES, SPP, jit)[0], ctx.mesh_trees()
    assert (frame != frame[0, 0]).any(), "the mesh is not in the frame"
    commits = ctx.skin(m)["device_commits"]
    ctx.set_mesh_bones(m, np.full((4, 12), 1e300))                   # overflows: a non-finite vertex
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame)
    huge = np.tile(np.array([1e295, 0, 0, 0, 0, 1e295, 0, 0, 0, 0, 1e295, 0]), (4, 1))   # finite vertices the transform takes past 1e300: the item loses its bounds
    assert np.isfinite(ft.skin_blend(base, index, weight, huge)).all()
    ctx.set_mesh_bones(m, huge)
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "bounds" in ctx.last_error()
    assert ctx.skin(m)["device_commits"] == commits + 2 and ctx.morph(m)["from_device"]
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame)
    same_trees(ctx.mesh_trees(), T1, "after two refused commits")
    bones2 = palette(4, 41, e.centre, e.radius)
    ctx.set_mesh_bones(m, bones2)                                    # and no state was lost: the next pose commits
    ctx.commit_deformed()
    m2 = build(twin, base)
    twin.set_mesh_triangles(m2, ft.skin_blend(base, index, weight, bones2))
    twin.commit_deformed()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])
    same_trees(ctx.mesh_trees(), twin.mesh_trees(), "the pose after the refusals")
    m = build(ctx, base, depth=1)                                    # depth 1: refused before any kernel runs
    frame = ctx.render(cam, RES, RES, SPP, jit)[0]
    ctx.set_mesh_skin(m, index, weight)
    ctx.set_mesh_bones(m, bones)
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "depth" in ctx.last_error()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame)


@pytest.mark.gpu
def test_queued_frames_see_the_pose_they_were_queued_under(contexts):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh, bvh_builder=3)
    e = CAT["blob(1025)"]
    base, index, weight, bones = pose_of(e, 4, 9, "equal")
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    cam, jit = B.camera(e.centre, 2.0 * e.radius), ft.jitter_pattern(SPP)
    old = ctx.render(cam, RES, RES, SPP, jit)[0]
    ctx.set_mesh_skin(rec.meshes[0], index, weight)
    for _ in range(3):
        ctx.render_enqueue(cam, RES, RES, SPP, jit)
    ctx.set_mesh_bones(rec.meshes[0], bones)
    ctx.commit_deformed()                                            # retires the three frames first: they traced the old pose
    assert same(ctx.fetch_frame(np.zeros((RES, RES, 3))), old), "the last frame queued before the commit is not the old pose's"
    for _ in range(2):
        ctx.render_enqueue(cam, RES, RES, SPP, jit)
    ctx.wait()
    B.build_scene(fresh, ft.skin_blend(base, index, weight, bones))
    assert same(ctx.fetch_frame(np.zeros((RES, RES, 3))), fresh.render(cam, RES, RES, SPP, jit)[0]), "a frame queued after the commit is not the new pose's"


@pytest.mark.gpu
def test_every_device_of_a_context_skins_its_copy(contexts):
    one = contexts("work")
    _options(one, bvh_builder=3)
    two = ft.Context(device=[0, 0])
    try:
        two.set_option("bvh_builder", 3)
        e = CAT["blob(1025)"]
        base, index, weight, bones = pose_of(e, 4, 30, "mixed")
        view = view_of(ft.skin_blend(base, index, weight, bones))
        out = []
        for c in (one, two):
            rec = Recorder(c)
            B.build_scene(rec, base)
            c.set_mesh_skin(rec.meshes[0], index, weight)
            c.set_mesh_bones(rec.meshes[0], bones)
            c.commit_deformed()
            assert c.morph(rec.meshes[0])["from_device"] and c.skin(rec.meshes[0])["device_meshes"] == 1
            out.append((c.render(B.camera(*view), RES, RES, SPP, ft.jitter_pattern(SPP))[0], c.mesh_trees()))
        assert same(out[0][0], out[1][0]), "the two devices' bands are not the single device's frame"
        same_trees(out[0][1], out[1][1], "two devices")
    finally:
        two.close()

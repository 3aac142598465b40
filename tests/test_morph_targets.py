"""Morph targets (ft_sg_set_mesh_targets / ft_sg_set_mesh_weights / ft_debug_morph): key shapes resident in device memory,
K weights per pose, the vertices blended by k_morph_blend into the buffer the refit reads and scanned there (ft_morph.hip).

The promise under test: set_mesh_weights(node, w) followed by any commit gives every bit that set_mesh_triangles(node, V) followed by the
same commit gives, V = functracer_amd.morph_blend(base, targets, w) - the formula of the header in numpy, one elementwise IEEE operation per
step.  Every comparison is bitwise; there is no tolerance in this file."""
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
from .test_mesh_refit import (CAT, RES, SPP, Recorder, _ground_scene, _owned, answers, assert_same_answers, assert_same_topology, contexts, deform,  # noqa: F401 (contexts: a fixture)
                              same)

TREE_KEYS = ("nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes")
KINDS = ("jitter", "twist", "far", "small")
GPU_MESHES = ["blob(7)", "blob(8)", "blob(65)", "blob(257)", "blob(1025)", "degenerate", "flat", "identical"]


def targets_of(e, k_targets):
    """k_targets key shapes of catalogue entry `e`: test_mesh_refit.deform's jitter / twist / far / small of the base, in turn, at growing amounts."""
    return np.stack([deform(e, KINDS[k % 4], 1.0 + 0.25 * (k // 4))[0] for k in range(k_targets)]).reshape(k_targets, -1, 9)


def weight_sets(k_targets):
    cancel = np.resize([1e16, 1.0, -1e16, 0.5], k_targets)           # partial sums that cancel: the order of the terms shows
    return {"zeros": np.zeros(k_targets), "ones": np.ones(k_targets), "mixed": np.resize([0.3, -1.5, 2.0], k_targets), "tiny": np.full(k_targets, 1e-300), "cancel": cancel}


def view_of(v):
    p = v.reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return 0.5 * (lo + hi), max(0.5 * float(np.linalg.norm(hi - lo)), 1e-3)


def same_trees(a, b, what, keys=TREE_KEYS):
    for k in keys:
        assert same(a[k], b[k]), f"{what}: {k} differs"


def replay_scan(v):
    """fth::scan_mesh in numpy: bounds over the nine coordinates of every triangle as given, the FIRST of equal values kept (-0.0 == +0.0,
    so a zero bound has the sign of the first zero in list order); extent over v0, v0 + (v1 - v0), v0 + (v2 - v0)."""
    t = v.reshape(-1, 9)
    p = t.reshape(-1, 3)                                             # list order: triangle, then corner
    out = np.zeros(7)
    for a in range(3):
        col = p[:, a]
        out[a] = col[np.flatnonzero(col == col.min())[0]]
        out[3 + a] = col[np.flatnonzero(col == col.max())[0]]
    v0 = t[:, 0:3]
    seen = np.stack([np.abs(v0), np.abs(v0 + (t[:, 3:6] - v0)), np.abs(v0 + (t[:, 6:9] - v0))])
    out[6] = max(0.0, float(seen.max()))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_bindings_declare_the_morph_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert "#define FT_MAX_MORPH_TARGETS 16" in hdr and "#define FT_ABI_VERSION 2" in hdr and '"morph_on_device"' in hdr
    assert re.search(r"int32_t ft_sg_set_mesh_targets\(ft_context\* ctx, ft_node mesh, const double\* targets, int32_t n_targets, int64_t n_tris\);", hdr)
    assert re.search(r"int32_t ft_sg_set_mesh_weights\(ft_context\* ctx, ft_node mesh, const double\* weights, int32_t n_weights\);", hdr)
    assert re.search(r"int32_t ft_debug_morph\(ft_context\* ctx, ft_node mesh, int64_t counts\[4\], double scan\[8\]\);", hdr)
    lib = C.CDLL(ft.HIP_LIB)
    doc = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    for name in ("ft_sg_set_mesh_targets", "ft_sg_set_mesh_weights", "ft_debug_morph"):
        assert hasattr(lib, name), name
        assert re.search(r"\[<DllImport\(Lib\)>\] extern int " + name + r"\(", doc), name
        assert name in [s[0] for s in _capi.MORPH_SIGNATURES]
    for name in ("set_mesh_targets", "set_mesh_weights", "morph"):
        assert callable(getattr(ft.Context, name)), name
    assert callable(ft.morph_blend) and _capi.MAX_MORPH_TARGETS == 16


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
    T0 = ctx.mesh_trees()
    e = CAT["blob(9)"]
    t2 = np.ascontiguousarray(targets_of(e, 2))
    t17 = np.ascontiguousarray(np.resize(t2, (17, 9, 9)))
    w = np.array([0.5, 0.25])
    p2, pw = _capi.dptr(t2), _capi.dptr(w)
    assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["flat"], pw, 2) == -1    # weights without targets
    assert lib.ft_sg_set_mesh_targets(None, hd["flat"], p2, 2, 9) == -1
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, -1, p2, 2, 9) == -1 and lib.ft_sg_set_mesh_targets(ctx._ctx, 10_000, p2, 2, 9) == -1
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["xf"], p2, 2, 9) == -1   # a transform node
    for n in (8, 10, 0, -1):
        assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["flat"], p2, 2, n) == -1, n
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["flat"], _capi.dptr(t17), 17, 9) == -1
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["flat"], p2, -1, 9) == -1
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["flat"], None, 2, 9) == -1
    assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["flat"], pw, 2) == -1    # every call above was refused: still no targets
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["flat"], p2, 2, 9) == 0
    assert lib.ft_sg_set_mesh_weights(None, hd["flat"], pw, 2) == -1
    assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["xf"], pw, 2) == -1
    assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["flat"], None, 2) == -1
    for n in (1, 3, 0, -1):
        assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["flat"], pw, n) == -1, n
    for bad in (np.nan, np.inf, -np.inf):
        assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["flat"], _capi.dptr(np.array([0.5, bad])), 2) == -1, bad
    counts, scan = (C.c_int64 * 4)(), np.zeros(8)
    assert lib.ft_debug_morph(ctx._ctx, hd["xf"], counts, _capi.dptr(scan)) == -1 and lib.ft_debug_morph(None, hd["flat"], counts, _capi.dptr(scan)) == -1
    ctx.commit_deformed()                                            # nothing was marked: the commit of before, bit for bit
    same_trees(ctx.mesh_trees(), T0, "after the refused calls")
    ctx.commit()
    same_trees(ctx.mesh_trees(), T0, "after the refused calls and a full commit")
    assert lib.ft_sg_set_mesh_targets(ctx._ctx, hd["flat"], None, 0, 9) == 0    # removes them
    assert lib.ft_sg_set_mesh_weights(ctx._ctx, hd["flat"], pw, 2) == -1
    ctx.close()


def test_morph_on_device_is_an_option_of_every_context():
    ctx = ft.Context(host_only=True)
    for v in (0, 1, 7, -1):
        ctx.set_option("morph_on_device", v)
    ctx.close()


def _fused(base, targets, w):
    """blend() with every step a fused multiply-add - what the library must NOT compute."""
    d = targets - base
    acc = base.copy()
    flat, out = d.reshape(d.shape[0], -1), acc.reshape(-1)
    for k in range(d.shape[0]):
        if hasattr(math, "fma"):
            out[:] = [math.fma(float(w[k]), float(x), float(a)) for x, a in zip(flat[k], out)]
        else:
            out[:] = [float(Fraction(float(w[k])) * Fraction(float(x)) + Fraction(float(a))) for x, a in zip(flat[k], out)]
    return acc


@pytest.mark.parametrize("name", ["blob(9)", "degenerate", "identical"])
def test_host_only_weights_give_the_bits_of_explicit_vertices(name):
    e = CAT[name]
    base = e.tris.reshape(-1, 9)
    ctx, twin, fresh = ft.Context(host_only=True), ft.Context(host_only=True), ft.Context(host_only=True)
    for k_targets in (1, 2, 16):
        targets = targets_of(e, k_targets)
        cases = list(weight_sets(k_targets).items())
        # targets several times the base's size plus noise: w * d has more than 53 significant bits and is of the sum's magnitude, so a fused
        # step (one rounding of the exact w * d + acc) differs from the two roundings the library promises
        big = base[None] * np.linspace(3.0, 7.0, k_targets)[:, None, None] + np.random.default_rng(5).uniform(-1.0, 1.0, size=(k_targets,) + base.shape)
        wbig = np.resize([1.0 / 3.0, -2.0 / 7.0], k_targets)
        assert (_fused(base, big, wbig) != ft.morph_blend(base, big, wbig)).any(), "the never-fused case is vacuous: fusing changes no bit of it"
        cases.append(("never-fused", wbig))
        for label, w in cases:
            tg = big if label == "never-fused" else targets
            what = f"{name}, K = {k_targets}, {label}"
            v = ft.morph_blend(base, tg, w)
            nodes = []
            for c in (ctx, twin):
                rec = Recorder(c)
                B.build_scene(rec, base)
                nodes.append(rec.meshes[0])
            ctx.set_mesh_targets(nodes[0], tg)
            ctx.set_mesh_weights(nodes[0], w)
            ctx.commit_deformed()
            twin.set_mesh_triangles(nodes[1], v)
            twin.commit_deformed()
            B.build_scene(fresh, v)
            got = ctx.mesh_trees()
            same_trees(got, twin.mesh_trees(), what + " (set_mesh_triangles)")
            same_trees(got, fresh.mesh_trees(), what + " (fresh graph)")
            m = ctx.morph(nodes[0])
            assert (m["device_meshes"], m["host_meshes"], m["from_device"], m["device_commits"], m["resident_bytes"]) == (0, 1, False, 0, 0), what
            assert same(m["scan"][:7], replay_scan(v)), what
    for c in (ctx, twin, fresh):
        c.close()


def test_the_vertices_are_blended_when_another_commit_needs_them():
    e = CAT["blob(65)"]
    base = e.tris.reshape(-1, 9)
    targets = targets_of(e, 3)
    ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)

    def build(b, tris, shift):
        b.clear()
        m = b.bsp_mesh(0, tris.reshape(-1, 9))
        xf = b.transform([("translate", (shift, 0, 0))], m)
        b.set_objects(b.group([xf]))
        b.add_directional((1, -2, 1), (1, 1, 1))
        b.commit()
        return m, xf

    def expect(tris, shift, what):
        build(fresh, tris, shift)
        same_trees(ctx.mesh_trees(), fresh.mesh_trees(), what)
        assert all(same(x, y) for x, y in zip(ctx.leaf_matrices(), fresh.leaf_matrices())), what
    m, xf = build(ctx, base, 0.0)
    ctx.set_mesh_targets(m, targets)
    w1, w2, w3 = [0.2, 0.0, 0.1], [0.0, 0.7, -0.3], [1.0, 1.0, 1.0]
    ctx.set_mesh_weights(m, w1)
    ctx.commit()                                                     # a plain full commit with weights pending
    expect(ft.morph_blend(base, targets, w1), 0.0, "weights, then ft_scene_commit")
    ctx.set_mesh_weights(m, w2)
    ctx.set_transform(xf, [("translate", (2.0, 0, 0))])
    ctx.commit_moved()                                               # a moved commit with weights pending: the full commit
    expect(ft.morph_blend(base, targets, w2), 2.0, "weights, then set_transform + ft_scene_commit_moved")
    explicit = deform(e, "twist", 0.3)[0]
    ctx.set_mesh_weights(m, w3)
    ctx.set_mesh_triangles(m, explicit)                              # explicit vertices win; base and deltas stay
    ctx.commit_deformed()
    expect(explicit, 2.0, "set_mesh_triangles after weights")
    ctx.set_mesh_weights(m, w3)
    ctx.commit_deformed()
    expect(ft.morph_blend(base, targets, w3), 2.0, "weights again: the base is still the one of set_mesh_targets")
    ctx.commit()
    expect(ft.morph_blend(base, targets, w3), 2.0, "a full commit after a weight commit")
    # new targets: the base is the vertices as they stand, the blended ones
    now = ft.morph_blend(base, targets, w3)
    ctx.set_mesh_targets(m, targets[:1])
    ctx.commit_deformed()                                            # nothing is marked deformed
    expect(now, 2.0, "set_mesh_targets alone changes no vertex")
    ctx.set_mesh_weights(m, [0.5])
    ctx.commit_deformed()
    expect(ft.morph_blend(now, targets[:1], [0.5]), 2.0, "weights over the new base")
    ctx.close(), fresh.close()


def test_a_weight_that_overflows_is_refused_and_the_old_commit_stays():
    ctx = ft.Context(host_only=True)
    e = CAT["blob(9)"]
    rec = Recorder(ctx)
    B.build_scene(rec, e.tris)
    T0 = ctx.mesh_trees()
    ctx.set_mesh_targets(rec.meshes[0], targets_of(e, 2))
    ctx.set_mesh_weights(rec.meshes[0], [1e308, 0.0])
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    same_trees(ctx.mesh_trees(), T0, "after the refused commit")
    ctx.set_mesh_weights(rec.meshes[0], [0.5, 0.5])
    ctx.commit_deformed()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _options(*ctxs, **opts):
    base = {"bvh_builder": 2, "primary_block_lists": 1, "light_space_shadows": 2, "deform_light_space": 0, "light_space_retree": 0, "refit_rebuild_percent": 0,
            "temporal_follow_deformed": 0, "morph_on_device": 1}
    base.update(opts)
    for c in ctxs:
        for k, v in base.items():
            c.set_option(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("k_targets", [1, 3, 16])
@pytest.mark.parametrize("name", GPU_MESHES)
@pytest.mark.parametrize("builder", [0, 3])
def test_weights_give_every_bit_that_explicit_vertices_give(contexts, builder, name, k_targets):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh, bvh_builder=builder)
    e = CAT[name]
    base, targets = e.tris.reshape(-1, 9), targets_of(e, k_targets)
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    node = rec.meshes[0]
    T0 = ctx.mesh_trees()
    ctx.set_mesh_targets(node, targets)
    commits = ctx.morph(node)["device_commits"]
    for label in ("mixed", "quarters"):
        w = weight_sets(k_targets)[label] if label == "mixed" else np.resize([0.75, 0.5, -0.75, 0.125], k_targets)
        what = f"builder {builder}, {name}, K = {k_targets}, {label}"
        v = ft.morph_blend(base, targets, w)
        view = view_of(v)
        ctx.set_option("morph_on_device", 1)
        ctx.set_mesh_weights(node, w)
        ctx.commit_deformed()
        m = ctx.morph(node)
        commits += 1
        assert (m["device_meshes"], m["host_meshes"], m["from_device"], m["device_commits"]) == (1, 0, True, commits), what
        assert m["resident_bytes"] == (k_targets + 1) * base.size * 8, what
        assert same(m["scan"][:7], replay_scan(v)), f"{what}: the device scan is not scan_mesh's"
        got, T1 = answers(ctx, view, v.reshape(-1, 3, 3)), ctx.mesh_trees()
        assert got["hit"].any() and (got["frame"] != got["frame"][0, 0]).any(), f"{what}: the mesh is not in the view"
        assert_same_topology(T0, T1, what)
        ctx.set_option("morph_on_device", 0)
        ctx.set_mesh_weights(node, w)
        ctx.commit_deformed()
        m = ctx.morph(node)
        assert (m["device_meshes"], m["host_meshes"], m["from_device"], m["device_commits"]) == (0, 1, False, commits), what
        assert same(m["scan"][:7], replay_scan(v)), what
        assert_same_answers(answers(ctx, view, v.reshape(-1, 3, 3)), got, what + " (morph_on_device 0)")
        same_trees(ctx.mesh_trees(), T1, what + " (morph_on_device 0)")
        ctx.set_mesh_triangles(node, v)
        ctx.commit_deformed()
        assert_same_answers(answers(ctx, view, v.reshape(-1, 3, 3)), got, what + " (set_mesh_triangles)")
        same_trees(ctx.mesh_trees(), T1, what + " (set_mesh_triangles)")
        B.build_scene(fresh, v)
        assert_same_answers(got, answers(fresh, view, v.reshape(-1, 3, 3)), what + " (fresh context)")
    ctx.set_option("morph_on_device", 1)


def _zero_mesh(first, second, at_first, at_second, n=600):
    """n triangles with x >= 0 and y <= 0 whose extreme x and y are zeros: `first` at triangle at_first, `second` at triangle at_second."""
    rng = np.random.default_rng(31)
    t = rng.uniform(0.25, 1.5, size=(n, 3, 3))
    t[:, :, 1] = -t[:, :, 1]
    for at, z in ((at_first, first), (at_second, second)):
        t[at, 1, 0] = z
        t[at, 2, 1] = z
    return t.reshape(-1, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["minus-first", "plus-first", "minus-first-across-blocks", "plus-first-across-blocks", "one-triangle"])
def test_a_zero_bound_has_the_sign_of_the_first_zero_in_the_list(contexts, case):
    ctx = contexts("work")
    _options(ctx)
    first = -0.0 if case.startswith("minus") else 0.0
    places = (100, 500) if case.endswith("blocks") else (10, 20)
    base = _zero_mesh(first, -first, *places)
    if case == "one-triangle":                                       # both zeros in one triangle: corner 0 before corner 1
        base = _zero_mesh(0.5, 0.5, 10, 20)
        base[10, 7] = base[20, 7] = -0.5
        base[300, 0], base[300, 3], base[300, 4], base[300, 7] = -0.0, 0.0, 0.0, -0.0
        first = -0.0
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    node = rec.meshes[0]
    # targets = the base, weight -1: every delta is +0.0 and every product -0.0, which added to a coordinate gives the coordinate, sign included
    w = [-1.0]
    v = ft.morph_blend(base, base[None], w)
    assert same(v, base) and np.signbit(v).any() and (v == 0.0).sum() >= 4
    ctx.set_mesh_targets(node, base[None])
    ctx.set_mesh_weights(node, w)
    ctx.commit_deformed()
    m = ctx.morph(node)
    want = replay_scan(v)
    assert m["from_device"] and same(m["scan"][:7], want), (m["scan"], want)
    assert m["scan"][0] == 0.0 and bool(np.signbit(m["scan"][0])) == bool(np.signbit(first)), "lower x bound: not the first zero's sign"
    y_first = 0.0 if case == "one-triangle" else first
    assert m["scan"][4] == 0.0 and bool(np.signbit(m["scan"][4])) == bool(np.signbit(y_first)), "upper y bound: not the first zero's sign"
    ctx.set_option("morph_on_device", 0)
    T1 = ctx.mesh_trees()
    ctx.set_mesh_weights(node, w)
    ctx.commit_deformed()
    same_trees(ctx.mesh_trees(), T1, case)
    assert same(ctx.morph(node)["scan"][:7], want)
    ctx.set_option("morph_on_device", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("retree", [0, 1])
@pytest.mark.parametrize("name", ["blob(257)", "blob(1025)"])
def test_light_space_structures_follow_the_weights(contexts, name, retree):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, deform_light_space=1, light_space_retree=retree)
    e = CAT[name]
    base, targets = e.tris.reshape(-1, 9), targets_of(e, 2)
    cam, jit = B.camera(e.centre, 2.0 * e.radius), ft.jitter_pattern(SPP)
    nodes = [_ground_scene(c, base) for c in (ctx, twin)]
    ctx.set_mesh_targets(nodes[0], targets)
    for w in ([0.4, 0.1], [0.1, 0.3]):
        v = ft.morph_blend(base, targets, w)
        ctx.set_mesh_weights(nodes[0], w)
        ctx.commit_deformed()
        assert ctx.morph(nodes[0])["from_device"]
        twin.set_mesh_triangles(nodes[1], v)
        twin.commit_deformed()
        got, want = light_space(ctx), light_space(twin)
        assert got[3][0] != 0xFFFFFFFF, "the caster's leaf lost its pairs"
        assert same(got[0][:, :14], want[0][:, :14]), "pair records [0..13]"
        for a, b, what in zip(got, want, ("pairs", "nodes and grids", "records", "leaf pairs")):
            assert same(a, b), what
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])
    _options(ctx, twin)


@pytest.mark.gpu
def test_two_morph_meshes_and_one_explicit_mesh_in_one_commit(contexts, monkeypatch):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh)
    rec = Recorder(ctx)
    B.build_multi(rec)
    node = {part[0]: h for part, h in zip(B.MULTI_PARTS, rec.meshes)}
    cam, jit = B.camera(*B.MULTI_VIEW), ft.jitter_pattern(SPP)
    T0 = ctx.mesh_trees()
    new = {}
    for name, w in (("blob(257)", [0.5, 0.02]), ("blob(1025)", [0.3, 0.05, 0.0])):
        base, targets = CAT[name].tris.reshape(-1, 9), targets_of(CAT[name], len(w))
        ctx.set_mesh_targets(node[name], targets)
        ctx.set_mesh_weights(node[name], w)
        new[name] = ft.morph_blend(base, targets, w).reshape(-1, 3, 3)
    new["blob(8)"] = deform(CAT["blob(8)"], "jitter")[0]
    ctx.set_mesh_triangles(node["blob(8)"], new["blob(8)"])
    ctx.commit_deformed()
    m = ctx.morph(node["blob(8)"])
    assert (m["device_meshes"], m["host_meshes"], m["from_device"]) == (2, 0, False)
    assert same(m["scan"][:7], replay_scan(new["blob(8)"]))
    for name in ("blob(257)", "blob(1025)"):
        m = ctx.morph(node[name])
        assert m["from_device"] and same(m["scan"][:7], replay_scan(new[name])), name
    assert not ctx.morph(node["blob(7)"])["scan"].any()
    T1 = ctx.mesh_trees()
    reports = B.check_trees(T1)
    assert [r["n"] for r in reports] == [8, 257, 1025]
    assert_same_topology(T0, T1, "multi")
    owned = [_owned(T1, r) for r in reports]
    for k in ("nodes", "tris", "wide", "coarse_boxes"):              # the untouched meshes' ranges keep every bit
        a, b = T0[k].view(np.uint8).reshape(T0[k].shape[0], -1), T1[k].view(np.uint8).reshape(T1[k].shape[0], -1)
        changed = set(np.nonzero((a != b).any(axis=1))[0].tolist())
        assert changed and changed <= set().union(*(o[k] for o in owned)), k
    frame = ctx.render(cam, RES, RES, SPP, jit)[0]
    # the same three edits as explicit vertices, and a fresh graph of them
    ctx2 = contexts("twin")
    _options(ctx2)
    rec2 = Recorder(ctx2)
    B.build_multi(rec2)
    for (part, h) in zip(B.MULTI_PARTS, rec2.meshes):
        if part[0] in new:
            ctx2.set_mesh_triangles(h, new[part[0]])
    ctx2.commit_deformed()
    same_trees(T1, ctx2.mesh_trees(), "weights against explicit vertices")
    assert same(frame, ctx2.render(cam, RES, RES, SPP, jit)[0])
    cat = dict(CAT)
    for name, t in new.items():
        cat[name] = CAT[name]._replace(tris=np.ascontiguousarray(t))
    monkeypatch.setattr(B, "catalogue", lambda: cat)
    B.build_multi(fresh)
    monkeypatch.undo()
    assert same(frame, fresh.render(cam, RES, RES, SPP, jit)[0]), "the frame is not the fresh context's"


@pytest.mark.gpu
@pytest.mark.parametrize("percent", [0, 100])
def test_six_weight_commits_in_a_row_then_a_full_commit(contexts, percent):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh, bvh_builder=3, refit_rebuild_percent=percent)
    fresh.set_option("refit_rebuild_percent", 0)
    e = CAT["blob(1025)"]
    base = e.tris.reshape(-1, 9)
    targets = np.stack([deform(e, "twist", 0.9)[0], deform(e, "jitter", 3.0)[0]]).reshape(2, -1, 9)
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    node = rec.meshes[0]
    ctx.set_mesh_targets(node, targets)
    cam, jit = B.camera(e.centre, 2.5 * e.radius), ft.jitter_pattern(SPP)
    for step in range(1, 7):
        w = [step / 6.0, 0.1 * step]
        ctx.set_mesh_weights(node, w)
        ctx.commit_deformed()
        assert ctx.morph(node)["device_commits"] >= step and ctx.morph(node)["from_device"]
        v = ft.morph_blend(base, targets, w)
        B.build_scene(fresh, v)
        want = fresh.render(cam, RES, RES, SPP, jit)[0]
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], want), f"step {step}"
    B.check_trees(ctx.mesh_trees())
    ctx.commit()                                                     # the host blends the vertices it never saw
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], want)
    same_trees(ctx.mesh_trees(), fresh.mesh_trees(), "the full commit after six weight commits")
    _options(ctx, fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("follow", [0, 1])
def test_the_temporal_accumulation_follows_weights_as_it_follows_vertices(contexts, follow):
    W, Hh, calls = 96, 64, 6
    e = CAT["blob(257)"]
    base = e.tris.reshape(-1, 9)
    targets = np.stack([deform(e, "jitter", 2.0)[0], deform(e, "twist", 0.2)[0]]).reshape(2, -1, 9)
    jit = np.zeros((1, 2))
    cams = [B.camera(e.centre + np.array([0.05 * k, 0.0, 0.0]), 2.0 * e.radius) for k in range(calls)]

    def run(ctx, by_weights):
        m = _ground_scene(ctx, base)
        if by_weights:
            ctx.set_mesh_targets(m, targets)
        ctx.temporal_begin(W, Hh)
        out = []
        for k, cam in enumerate(cams):
            if k:
                w = [0.0, 0.0] if k < 3 else [0.25 * (k - 2), 0.1 * (k - 2)]
                if by_weights:
                    ctx.set_mesh_weights(m, w)
                else:
                    ctx.set_mesh_triangles(m, ft.morph_blend(base, targets, w))
                ctx.commit_deformed()
            ctx.render(cam, W, Hh, 1, jit, seed=100 + k, fetch=False)
            ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
            out.append(([np.asarray(a).tobytes() for a in ctx.temporal_fetch()], ctx.temporal_status()))
        ctx.temporal_end()
        return out
    _options(contexts("work"), contexts("fresh"), temporal_follow_deformed=follow)
    explicit, weights = run(contexts("fresh"), False), run(contexts("work"), True)
    assert explicit == weights and weights[-1][1]["calls"] == calls
    _options(contexts("work"), contexts("fresh"))


@pytest.mark.gpu
def test_refusals_on_the_device_leave_the_old_commit(contexts):
    ctx = contexts("work")
    _options(ctx)
    e = CAT["blob(257)"]
    base = e.tris.reshape(-1, 9)
    cam, jit = B.camera(1e6 * e.centre, 3e6 * e.radius), ft.jitter_pattern(SPP)   # (the scene is the mesh a million times its size)

    def build(tris):
        ctx.clear()
        m = ctx.bsp_mesh(0, tris)
        ctx.set_objects(ctx.group([ctx.transform([("scale", (1e6, 1e6, 1e6))], ctx.material(m, colour=(0.9, 0.5, 0.2)))]))
        ctx.add_directional((1, -2, 1), (1, 1, 1))
        ctx.commit()
        return m
    m = build(base)
    ctx.set_mesh_targets(m, np.stack([base * 2.0, base * 1e295]))
    ctx.set_mesh_weights(m, [0.5, 0.0])
    ctx.commit_deformed()
    frame, T1 = ctx.render(cam, RES, RES, SPP, jit)[0], ctx.mesh_trees()
    assert (frame != frame[0, 0]).any(), "the mesh is not in the frame"
    commits = ctx.morph(m)["device_commits"]
    ctx.set_mesh_weights(m, [1e308, 0.0])                            # overflows: a non-finite vertex
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame)
    ctx.set_mesh_weights(m, [0.0, 1.0])                              # finite vertices of 1e295 that the transform takes past 1e300: the item loses its bounds
    assert np.isfinite(ft.morph_blend(base, np.stack([base * 2.0, base * 1e295]), [0.0, 1.0])).all()
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "bounds" in ctx.last_error()
    assert ctx.morph(m)["device_commits"] == commits + 2 and ctx.morph(m)["from_device"]
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame)
    same_trees(ctx.mesh_trees(), T1, "after two refused commits")
    ctx.set_mesh_weights(m, [0.25, 0.0])                             # and no state was lost: the next pose commits
    ctx.commit_deformed()
    twin = contexts("fresh")
    _options(twin)
    ctx, keep = twin, ctx
    m2 = build(base)
    twin.set_mesh_triangles(m2, ft.morph_blend(base, np.stack([base * 2.0, base * 1e295]), [0.25, 0.0]))
    twin.commit_deformed()
    assert same(keep.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])
    same_trees(keep.mesh_trees(), twin.mesh_trees(), "the pose after the refusals")


@pytest.mark.gpu
def test_queued_frames_see_the_pose_they_were_queued_under(contexts):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh, bvh_builder=3)
    e = CAT["blob(1025)"]
    base, targets = e.tris.reshape(-1, 9), targets_of(e, 2)
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    cam, jit = B.camera(e.centre, 2.0 * e.radius), ft.jitter_pattern(SPP)
    old = ctx.render(cam, RES, RES, SPP, jit)[0]
    ctx.set_mesh_targets(rec.meshes[0], targets)
    for _ in range(3):
        ctx.render_enqueue(cam, RES, RES, SPP, jit)
    w = [0.3, 0.2]
    ctx.set_mesh_weights(rec.meshes[0], w)
    ctx.commit_deformed()                                            # retires the three frames first: they traced the old pose
    assert same(ctx.fetch_frame(np.zeros((RES, RES, 3))), old), "the last frame queued before the commit is not the old pose's"
    for _ in range(2):
        ctx.render_enqueue(cam, RES, RES, SPP, jit)
    ctx.wait()
    B.build_scene(fresh, ft.morph_blend(base, targets, w))
    assert same(ctx.fetch_frame(np.zeros((RES, RES, 3))), fresh.render(cam, RES, RES, SPP, jit)[0]), "a frame queued after the commit is not the new pose's"


@pytest.mark.gpu
def test_every_device_of_a_context_blends_its_copy(contexts):
    one = contexts("work")
    _options(one, bvh_builder=3)
    two = ft.Context(device=[0, 0])
    try:
        two.set_option("bvh_builder", 3)
        e = CAT["blob(1025)"]
        base, targets = e.tris.reshape(-1, 9), targets_of(e, 3)
        w = [0.2, 0.1, 0.0]
        view = view_of(ft.morph_blend(base, targets, w))
        out = []
        for c in (one, two):
            rec = Recorder(c)
            B.build_scene(rec, base)
            c.set_mesh_targets(rec.meshes[0], targets)
            c.set_mesh_weights(rec.meshes[0], w)
            c.commit_deformed()
            assert c.morph(rec.meshes[0])["from_device"]
            out.append((c.render(B.camera(*view), RES, RES, SPP, ft.jitter_pattern(SPP))[0], c.mesh_trees()))
        assert same(out[0][0], out[1][0]), "the two devices' bands are not the single device's frame"
        same_trees(out[0][1], out[1][1], "two devices")
    finally:
        two.close()

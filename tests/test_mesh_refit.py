"""ft_sg_set_mesh_triangles / ft_scene_commit_deformed (Context.set_mesh_triangles / commit_deformed): the vertices of `bspMesh 0` meshes
of a committed scene change, the trees keep their topology and are refit on the device (ft_refit.hip).  A refit tree is held
to the standard of every builder here: what is read back from HBM passes tests/bvh_tools.check_trees, and frames, surface planes and ray
queries are bitwise those of a fresh context whose graph was built with the new vertices and committed with ft_scene_commit.

Deformations of a catalogue mesh: (a) Gaussian jitter of 1 % of the mesh radius, (b) a twist plus a stretch to 3x the original bounds (a
stale cull sphere or coarse box would clip the mesh), (c) every triangle moved onto the first one (boxes of zero extent), (d) a
translation by 1e3 on every axis (the pad grows with the extent), (e) a scale by 1 / 256."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import bvh_tools as B
from . import helpers as H
from .test_light_space_shadows import light_space

CAT = B.catalogue()
MESHES = ["blob(7)", "blob(8)", "blob(9)", "blob(65)", "blob(257)", "blob(1025)", "degenerate", "flat", "identical", "two_clusters"]
DEFORMS = ["jitter", "twist", "collapse", "far", "small"]
RES, SPP = 96, 4
NONE = 0xFFFFFFFF


def deform(e, how, amount=1.0):
    """(tris, centre, radius) of catalogue entry `e` after deformation `how`: the new vertices and where its dense part now is."""
    t = e.tris.copy()
    if how == "jitter":
        return t + np.random.default_rng(21).normal(size=t.shape) * 0.01 * e.radius * amount, e.centre, e.radius
    if how == "twist":
        p = t.reshape(-1, 3)
        lo, hi = p.min(axis=0), p.max(axis=0)
        c, half = 0.5 * (lo + hi), np.maximum(0.5 * (hi - lo), 1e-300)

        def f(q):
            r = q - c
            ang = 1.0 * amount * r[..., 1] / half[1]
            x, z = np.cos(ang) * r[..., 0] + np.sin(ang) * r[..., 2], -np.sin(ang) * r[..., 0] + np.cos(ang) * r[..., 2]
            return c + (1.0 + 2.0 * min(amount, 1.0)) * np.stack([x, r[..., 1], z], axis=-1)
        return f(t), f(e.centre), 3.0 * e.radius
    if how == "collapse":
        t[:] = t[0]
        return t, t[0].mean(axis=0), max(0.5 * float(np.linalg.norm(np.ptp(t[0], axis=0))), 1e-3)
    if how == "far":
        return t + 1e3, e.centre + 1e3, e.radius
    assert how == "small"
    return t / 256.0, e.centre / 256.0, e.radius / 256.0


class Recorder:
    """A builder that notes the handles bsp_mesh returns (bvh_tools' scene builders do not hand them out)."""

    def __init__(self, ctx):
        self._b, self.meshes = ctx, []

    def bsp_mesh(self, depth, tris):
        self.meshes.append(self._b.bsp_mesh(depth, tris))
        return self.meshes[-1]

    def __getattr__(self, name):
        return getattr(self._b, name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def answers(ctx, view, tris, rays=True):
    """What the tests compare bit for bit: the frame, render_aov's t / leaf / triangle planes, closest and blocked over rays_for's rays."""
    cam, jit = B.camera(*view), ft.jitter_pattern(SPP)
    out = {"frame": ctx.render(cam, RES, RES, SPP, jit)[0]}
    aov = ctx.render_aov(cam, RES, RES, SPP, jit, channels=["t", "leaf", "triangle"])
    out.update({k: aov[k] for k in ("t", "leaf", "triangle")})
    if rays:
        o, d, md = B.rays_for(view, tris, n=20000)
        for k, v in zip(("hit", "ct", "cp", "cn", "cc"), ctx.closest(o, d)):
            out[k] = v
        out["blocked"] = ctx.blocked(o, d, md)
    return out


def assert_same_answers(got, want, what):
    for k in want:
        assert same(got[k], want[k]), f"{what}: {k} differs from the fresh context's ({int((_bits(got[k]) != _bits(want[k])).sum())} bytes)"


@pytest.fixture(scope="module")
def contexts():
    """The device contexts the GPU tests share: 'work' is edited and refit, 'fresh' is cleared and rebuilt from new vertices every time."""
    made = {}

    def get(name, device=0):
        if name not in made:
            made[name] = ft.Context(device=device)
        return made[name]
    yield get
    for c in made.values():
        c.close()


_FRESH = {}


def fresh_answers(get, builder, name, how):
    """A fresh graph of the deformed vertices, committed with ft_scene_commit under the default options: once per (builder, mesh, deformation)."""
    key = (builder, name, how)
    if key not in _FRESH:
        ctx = get("fresh")
        tris, centre, radius = deform(CAT[name], how)
        for k, v in (("bvh_builder", builder), ("primary_block_lists", 1), ("light_space_shadows", 2)):
            ctx.set_option(k, v)
        B.build_scene(ctx, tris)
        _FRESH[key] = (answers(ctx, (centre, radius), tris), ctx.mesh_trees())
    return _FRESH[key]


def list_range(T, mesh=0):
    root = int(T["meshes"][mesh, 0])
    assert root < 0
    first, n = (int(x) for x in T["bsp_leaves"][~root])
    return first, n


def assert_same_topology(T0, T1, what):
    for k in ("left", "right", "axis"):
        assert np.array_equal(T0["nodes"][k], T1["nodes"][k]), f"{what}: nodes.{k} changed"
    for k in ("bsp_leaves", "tri_orig", "tri_src", "meshes"):
        assert np.array_equal(T0[k], T1[k]), f"{what}: {k} changed"
    assert np.array_equal(B._wide_children(T0), B._wide_children(T1)), f"{what}: the 4-wide children changed"
    assert T0["jobs"] == T1["jobs"] and T0["stack_capacity"] == T1["stack_capacity"], what


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_the_deform_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"int32_t ft_sg_set_mesh_triangles\(ft_context\* ctx, ft_node node, const double\* tris, int64_t n_tris\);", hdr)
    assert re.search(r"int32_t ft_scene_commit_deformed\(ft_context\* ctx\);", hdr)
    assert "#define FT_ABI_VERSION 2" in hdr
    lib = C.CDLL(ft.HIP_LIB)
    doc = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    for name in ("ft_sg_set_mesh_triangles", "ft_scene_commit_deformed"):
        assert hasattr(lib, name), name
        assert re.search(r"\[<DllImport\(Lib\)>\] extern int " + name + r"\(", doc), name
    for name in ("set_mesh_triangles", "commit_deformed"):
        assert callable(getattr(ft.Context, name)) and not hasattr(_capi.SceneBuilder, name), name


def _small(ctx):
    """A `bspMesh 0`, a depth-2 mesh and a cube under a transform; returns the handles."""
    ctx.clear()
    hd = {"flat": ctx.bsp_mesh(0, CAT["blob(9)"].tris.reshape(-1, 9)), "deep": ctx.bsp_mesh(2, CAT["blob(63)"].tris.reshape(-1, 9))}
    hd["xf"] = ctx.transform([("translate", (3, 0, 0))], ctx.primitive(ft.CUBE))
    ctx.set_objects(ctx.group([hd["flat"], ctx.transform([("translate", (0, 3, 0))], hd["deep"]), hd["xf"]]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    ctx.commit()
    return hd


def test_set_mesh_triangles_refuses_bad_arguments_and_changes_nothing():
    ctx = ft.Context(host_only=True)
    hd = _small(ctx)
    old, info = ctx.leaf_matrices(), ctx.scene_info()
    lib = ft.hip_lib()
    t = np.ascontiguousarray(CAT["blob(9)"].tris.reshape(-1, 9) + 1.0)
    p = _capi.dptr(t)
    assert lib.ft_sg_set_mesh_triangles(None, hd["flat"], p, 9) == -1
    assert lib.ft_sg_set_mesh_triangles(ctx._ctx, -1, p, 9) == -1 and lib.ft_sg_set_mesh_triangles(ctx._ctx, 10_000, p, 9) == -1
    assert lib.ft_sg_set_mesh_triangles(ctx._ctx, hd["xf"], p, 9) == -1                 # a transform node
    assert lib.ft_sg_set_mesh_triangles(ctx._ctx, hd["flat"], None, 9) == -1
    for n in (8, 10, 0, -1):
        assert lib.ft_sg_set_mesh_triangles(ctx._ctx, hd["flat"], p, n) == -1, n
    assert ctx.scene_info() == info                                  # still committed: the refused calls changed nothing
    assert all(same(x, y) for x, y in zip(ctx.leaf_matrices(), old))
    ctx.commit_deformed()
    assert ctx.scene_info() == info and all(same(x, y) for x, y in zip(ctx.leaf_matrices(), old))
    ctx.close()


def test_commit_deformed_refuses_out_of_order_calls():
    ctx = ft.Context(host_only=True)
    lib = ft.hip_lib()
    assert lib.ft_scene_commit_deformed(None) == -1
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -5              # no commit
    hd = _small(ctx)
    old = ctx.leaf_matrices()
    ctx.primitive(ft.SPHERE)
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -5              # a node was added
    ctx.commit()
    ctx.add_directional((1, 0, 0), (1, 1, 1))
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -5              # a light was added
    ctx.commit()
    ctx.set_transform(hd["xf"], [("translate", (4, 0, 0))])
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -5              # a transform is pending
    assert "ft_scene_commit_moved" in ctx.last_error()
    assert same(ctx.leaf_matrices()[0], old[0])                     # nothing was committed
    ctx.commit_moved()
    ctx.set_mesh_triangles(hd["flat"], CAT["blob(9)"].tris * 2.0)
    ctx.commit_deformed()                                            # and then the deformation
    ctx.set_option("light_space_shadows", 0)
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -5              # a commit-time option is pending
    ctx.close()


def test_commit_deformed_refuses_what_cannot_be_refit_and_keeps_the_old_commit():
    ctx = ft.Context(host_only=True)
    hd = _small(ctx)
    old, info = ctx.leaf_matrices(), ctx.scene_info()
    lib = ft.hip_lib()
    ctx.set_mesh_triangles(hd["deep"], CAT["blob(63)"].tris * 1.5)
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "depth" in ctx.last_error()
    assert all(same(x, y) for x, y in zip(ctx.leaf_matrices(), old)) and ctx.scene_info() == info
    ctx.commit()                                                     # ft_scene_commit handles it
    old, info = ctx.leaf_matrices(), ctx.scene_info()
    bad = CAT["blob(9)"].tris.copy()
    bad[4, 1, 2] = np.nan
    ctx.set_mesh_triangles(hd["flat"], bad)
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    assert all(same(x, y) for x, y in zip(ctx.leaf_matrices(), old)) and ctx.scene_info() == info
    bad[4, 1, 2] = np.inf
    ctx.set_mesh_triangles(hd["flat"], bad)
    assert lib.ft_scene_commit_deformed(ctx._ctx) == -4
    ctx.set_mesh_triangles(hd["flat"], CAT["blob(9)"].tris)
    ctx.commit_deformed()
    ctx.close()


@pytest.mark.parametrize("how", DEFORMS)
def test_host_only_commit_deformed_gives_the_fresh_commits_trees(how):
    ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)
    for name in ("blob(7)", "blob(65)", "degenerate"):
        rec = Recorder(ctx)
        B.build_scene(rec, CAT[name].tris)
        tris = deform(CAT[name], how)[0]
        ctx.set_mesh_triangles(rec.meshes[0], tris)
        ctx.commit_deformed()
        T = ctx.mesh_trees()
        B.check_trees(T)
        B.build_scene(fresh, tris)
        F = fresh.mesh_trees()
        for k in ("nodes", "bsp_leaves", "tris", "tri_orig", "wide", "coarse_boxes", "meshes"):
            assert same(T[k], F[k]), (name, k)
    ctx.close(), fresh.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _refit(get, builder, name, how, pbl=1, lss=2):
    """The work context: the catalogue mesh committed under the options, then deformed and refit.  Returns (ctx, trees before, view, tris)."""
    ctx = get("work")
    for k, v in (("bvh_builder", builder), ("primary_block_lists", pbl), ("light_space_shadows", lss)):
        ctx.set_option(k, v)
    rec = Recorder(ctx)
    B.build_scene(rec, CAT[name].tris)
    T0 = ctx.mesh_trees()
    tris, centre, radius = deform(CAT[name], how)
    ctx.set_mesh_triangles(rec.meshes[0], tris)
    ctx.commit_deformed()
    return ctx, T0, (centre, radius), tris


@pytest.mark.gpu
@pytest.mark.parametrize("how", DEFORMS)
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("builder", [0, 1, 3])
def test_refit_trees_pass_the_checker_and_keep_their_topology(contexts, builder, name, how):
    ctx, T0, _, tris = _refit(contexts, builder, name, how)
    T1 = ctx.mesh_trees()
    assert T1["from_device"]
    reports = B.check_trees(T1, replays=None)
    assert len(reports) == (0 if name == "blob(7)" else 1) and all(r["device_built"] == (builder != 0) for r in reports)
    assert_same_topology(T0, T1, f"{name} {how}")
    F = fresh_answers(contexts, builder, name, how)[1]
    first, n = list_range(T1)
    assert (first, n) == list_range(F) and n == tris.shape[0]
    assert same(T1["tris"][first:first + n], F["tris"][first:first + n]), "a list-order record is not the fresh context's"


@pytest.mark.gpu
@pytest.mark.parametrize("lss", [0, 2])
@pytest.mark.parametrize("pbl", [0, 1])
@pytest.mark.parametrize("how", DEFORMS)
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("builder", [0, 1, 3])
def test_refit_results_are_the_fresh_contexts(contexts, builder, name, how, pbl, lss):
    ctx, _, view, tris = _refit(contexts, builder, name, how, pbl, lss)
    want = fresh_answers(contexts, builder, name, how)[0]
    assert_same_answers(answers(ctx, view, tris), want, f"builder {builder} {name} {how} lists {pbl} light-space {lss}")


def _owned(T, report):
    """The indices of every array that belong to the checked mesh `report` describes."""
    own = {k: set() for k in ("nodes", "tris", "wide", "coarse_boxes")}
    own["nodes"] = {r for r in report["need"] if r >= 0}
    own["tris"] = set(range(report["first_global"], report["first_global"] + report["n"]))
    for r in report["leaf_refs"]:
        f, c = (int(x) for x in T["bsp_leaves"][~r])
        own["tris"] |= set(range(f, f + c))
    wc, stack = B._wide_children(T), [int(T["meshes"][report["mesh"], 3])]
    while stack:
        w = stack.pop()
        own["wide"].add(w)
        stack.extend(int(c) for c in wc[w] if c >= 0)
    cf, cc = (int(x) for x in T["meshes"][report["mesh"], 4:6])
    own["coarse_boxes"] = set(range(cf, cf + cc))
    return own


@pytest.mark.gpu
def test_refit_of_some_meshes_of_a_scene_leaves_the_others_alone(contexts, monkeypatch):
    ctx, fresh = contexts("work"), contexts("fresh")
    for c in (ctx, fresh):
        for k, v in (("bvh_builder", 2), ("primary_block_lists", 1), ("light_space_shadows", 2)):
            c.set_option(k, v)
    rec = Recorder(ctx)
    B.build_multi(rec)
    node = {part[0]: h for part, h in zip(B.MULTI_PARTS, rec.meshes)}
    cam, jit = B.camera(*B.MULTI_VIEW), ft.jitter_pattern(SPP)
    T0 = ctx.mesh_trees()
    new = {name: deform(CAT[name], how)[0] for name, how in (("blob(257)", "jitter"), ("blob(1025)", "twist"))}
    new["blob(1025)"] = CAT["blob(1025)"].tris + 0.3 * (new["blob(1025)"] - CAT["blob(1025)"].tris)   # (stays in the view)
    for name, t in new.items():
        ctx.set_mesh_triangles(node[name], t)
    ctx.commit_deformed()
    T1 = ctx.mesh_trees()
    reports = B.check_trees(T1)
    assert [r["n"] for r in reports] == [8, 257, 1025]
    assert_same_topology(T0, T1, "multi")
    owned = [_owned(T1, r) for r in reports if r["n"] in (257, 1025)]
    for k in ("nodes", "tris", "wide", "coarse_boxes"):
        a, b = _bits(T0[k]).reshape(T0[k].shape[0], -1), _bits(T1[k]).reshape(T1[k].shape[0], -1)
        changed = set(np.nonzero((a != b).any(axis=1))[0].tolist())
        assert changed and changed <= owned[0][k] | owned[1][k], f"{k}: records outside the edited meshes changed: {sorted(changed - owned[0][k] - owned[1][k])[:5]}"

    def fresh_frame(tris_of):
        cat = dict(CAT)
        for name, t in tris_of.items():
            cat[name] = CAT[name]._replace(tris=np.ascontiguousarray(t))
        monkeypatch.setattr(B, "catalogue", lambda: cat)
        B.build_multi(fresh)
        monkeypatch.undo()
        return fresh.render(cam, RES, RES, SPP, jit)[0]

    frame = ctx.render(cam, RES, RES, SPP, jit)[0]
    assert same(frame, fresh_frame(new)), "the frame after the refit is not the fresh context's"
    # the depth-3 mesh cannot be refit: refused, the old commit still renders, ft_scene_commit takes over
    new["blob(63)"] = deform(CAT["blob(63)"], "jitter")[0]
    ctx.set_mesh_triangles(node["blob(63)"], new["blob(63)"])
    with pytest.raises(ft.FtError) as e:
        ctx.commit_deformed()
    assert e.value.status == -4
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame), "the refused commit_deformed did not leave the old commit renderable"
    ctx.commit()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], fresh_frame(new))


@pytest.mark.gpu
def test_one_mesh_node_under_two_transforms_is_refit_for_both_leaves(contexts):
    ctx, fresh = contexts("work"), contexts("fresh")

    def build(b, tris):
        b.clear()
        m = b.bsp_mesh(0, tris.reshape(-1, 9))
        b.set_objects(b.group([b.transform([("translate", (-1.5, 0, 0))], b.material(m, colour=(0.9, 0.5, 0.2))),
                               b.transform([("rotate", (0, 1, 0), 0.8), ("scale", (0.6, 1.2, 0.6)), ("translate", (1.5, 0, 0.5))], m)]))
        b.add_directional((1, -2, 1), (1, 1, 1))
        b.commit()
        return m
    for c in (ctx, fresh):
        for k, v in (("bvh_builder", 2), ("primary_block_lists", 1), ("light_space_shadows", 2)):
            c.set_option(k, v)
    cam, jit = B.camera(np.zeros(3), 3.0), ft.jitter_pattern(SPP)
    m = build(ctx, CAT["blob(257)"].tris)
    tris = deform(CAT["blob(257)"], "twist", 0.4)[0]
    ctx.set_mesh_triangles(m, tris)
    ctx.commit_deformed()
    build(fresh, tris)
    got, want = ctx.render(cam, RES, RES, SPP, jit)[0], fresh.render(cam, RES, RES, SPP, jit)[0]
    assert same(got, want)
    leaf = ctx.render_aov(cam, RES, RES, SPP, jit, channels=["leaf"])["leaf"]
    assert (leaf == 0).any() and (leaf == 1).any(), "both instances are in the frame"


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, 3])
def test_five_refits_in_a_row_then_a_full_commit(contexts, builder):
    ctx, fresh = contexts("work"), contexts("fresh")
    for c in (ctx, fresh):
        for k, v in (("bvh_builder", builder), ("primary_block_lists", 1), ("light_space_shadows", 2)):
            c.set_option(k, v)
    e = CAT["blob(1025)"]
    rec = Recorder(ctx)
    B.build_scene(rec, e.tris)
    assert light_space(ctx)[3][0] != NONE
    cam, jit = B.camera(e.centre, 1.5 * e.radius), ft.jitter_pattern(SPP)
    for step in range(1, 6):
        tris = deform(e, "twist", 0.15 * step)[0]
        ctx.set_mesh_triangles(rec.meshes[0], tris)
        ctx.commit_deformed()                                        # a refit of the previous refit's tree
        B.build_scene(fresh, tris)
        got, want = ctx.render(cam, RES, RES, SPP, jit)[0], fresh.render(cam, RES, RES, SPP, jit)[0]
        assert same(got, want), f"refit {step}"
        assert light_space(ctx)[3][0] == NONE, "the edited mesh's leaf keeps light-space pairs that were not refit"
    B.check_trees(ctx.mesh_trees())
    ctx.commit()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], want)
    sizes_now, sizes_fresh = [a.shape for a in light_space(ctx)], [a.shape for a in light_space(fresh)]
    assert light_space(ctx)[3][0] != NONE and sizes_now == sizes_fresh and sizes_now[0][0] >= 1, "the full commit brings the light-space pairs back"


def _ground_scene(b, tris):
    b.clear()
    m = b.bsp_mesh(0, tris.reshape(-1, 9))
    ground = b.transform([("scale", (40.0, 1.0, 40.0)), ("translate", (-20.0, -3.0, -20.0))], b.primitive(ft.SQUARE))
    b.set_objects(b.group([b.material(m, colour=(0.9, 0.5, 0.2), shineyness=4.0), b.material(ground, colour=(0.5, 0.5, 0.5))]))
    b.add_directional((1, -2, 1), (1, 1, 1))
    b.commit()
    return m


@pytest.mark.gpu
def test_temporal_accumulation_survives_commit_deformed(contexts):
    W, Hh, calls = 96, 64, 6
    e = CAT["blob(257)"]
    jit = np.zeros((1, 2))
    cams = [B.camera(e.centre + np.array([0.05 * k, 0.0, 0.0]), 2.0 * e.radius) for k in range(calls)]

    def run(ctx, between):
        m = _ground_scene(ctx, e.tris)
        ctx.temporal_begin(W, Hh)
        out = []
        for k, cam in enumerate(cams):
            if k:
                between(ctx, m, k)
            ctx.render(cam, W, Hh, 1, jit, seed=100 + k, fetch=False)
            ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
            out.append((ctx.temporal_fetch(), ctx.temporal_status()))
        ctx.temporal_end()
        return out

    def same_vertices(ctx, m, k):
        ctx.set_mesh_triangles(m, e.tris)
        ctx.commit_deformed()
    for c in (contexts("fresh"), contexts("work")):
        for k, v in (("bvh_builder", 2), ("primary_block_lists", 1), ("light_space_shadows", 2)):
            c.set_option(k, v)
    plain = run(contexts("fresh"), lambda *a: None)
    refit = run(contexts("work"), same_vertices)
    for k, ((f0, s0), (f1, s1)) in enumerate(zip(plain, refit)):
        assert s0 == s1 and s0["calls"] == k + 1, k
        assert all(same(x, y) for x, y in zip(f0, f1)), f"call {k}: M, Q or N differ from the sequence without commit_deformed"

    # a real deformation half way, under a camera that stands still: the count goes on, the ground away from the mesh and its shadow keeps its history
    ctx = contexts("work")
    cam = cams[0]
    moved = deform(e, "jitter", 2.0)[0]

    def real(ctx, m, k):
        if k == 3:
            ctx.set_mesh_triangles(m, moved)
            ctx.commit_deformed()
    cams = [cam] * calls
    out = run(ctx, real)
    assert out[-1][1]["calls"] == calls
    _ground_scene(ctx, e.tris)
    before = (ctx.render(cam, W, Hh, 1, jit)[0], ctx.render_aov(cam, W, Hh, 1, jit, channels=["leaf"])["leaf"])
    _ground_scene(ctx, moved)
    after = (ctx.render(cam, W, Hh, 1, jit)[0], ctx.render_aov(cam, W, Hh, 1, jit, channels=["leaf"])["leaf"])
    steady = (before[1] == 1) & (after[1] == 1) & (_bits(before[0]).reshape(Hh, W, -1) == _bits(after[0]).reshape(Hh, W, -1)).all(axis=2)
    assert steady.sum() > 500
    # N of a pixel is 1 + the bilinear mean of its valid taps' N (include/functracer_hip.h): under a camera that stands still a pixel taps
    # itself with weight 1 - O(ulp) and its neighbours with the rest, and the ground the mesh uncovered at call 3 restarts at N = 1.  So N
    # grows by one per call exactly where no restarted pixel is within reach - one pixel per call since the deformation - and by one less a
    # few ulp beside one.
    lengths = [o[0][2] for o in out]
    far = steady.copy()
    for _ in range(calls - 3):                                       # erode: one pixel per call after the deformation
        pad = np.pad(far, 1, constant_values=False)
        far = np.logical_and.reduce([pad[1 + dy:1 + dy + Hh, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    print(f"steady ground pixels {int(steady.sum())}, of them out of reach of a restarted pixel {int(far.sum())}; N after the last call: min over steady "
          f"{lengths[-1][steady].min()!r}, pixels with N != {calls}: {int((lengths[-1][steady] != calls).sum())}")
    for k in range(1, calls):
        assert (lengths[k][steady] > lengths[k - 1][steady]).all(), f"call {k}: a ground pixel off the mesh and off its shadow did not keep N growing"
        assert (lengths[k][steady] > k + 1 - 1e-6).all(), f"call {k}: a ground pixel off the mesh and off its shadow lost its history"
    # (the mean of four taps that all hold k is k up to the rounding of its weights: a few ulp)
    assert far.any() and (np.abs(lengths[-1][far] - calls) <= 1e-9).all(), "ground pixels away from the mesh and its shadow do not hold one sample per call"


@pytest.mark.gpu
def test_commit_deformed_ends_a_progressive_accumulation(contexts):
    ctx = contexts("work")
    e = CAT["blob(65)"]
    rec = Recorder(ctx)
    B.build_scene(rec, e.tris)
    cam, jit = B.camera(e.centre, e.radius), ft.jitter_pattern(SPP)
    ctx.progressive_begin(cam, RES, RES)
    ctx.progressive_pass(SPP, jit)
    ctx.set_mesh_triangles(rec.meshes[0], deform(e, "jitter")[0])
    ctx.commit_deformed()
    st = _capi.ft_stats()
    assert ctx._lib.ft_progressive_pass(ctx._ctx, SPP, _capi.dptr(jit), 1, 0, None, C.byref(st)) == -5


@pytest.mark.gpu
def test_queued_frames_are_retired_before_the_refit(contexts):
    ctx = contexts("work")
    for k, v in (("bvh_builder", 3), ("primary_block_lists", 1), ("light_space_shadows", 2)):
        ctx.set_option(k, v)
    e = CAT["blob(1025)"]
    rec = Recorder(ctx)
    B.build_scene(rec, e.tris)
    cam0, jit = B.camera(e.centre, e.radius), ft.jitter_pattern(SPP)
    for _ in range(3):
        ctx.render_enqueue(cam0, RES, RES, SPP, jit)
    tris, centre, radius = deform(e, "twist")
    ctx.set_mesh_triangles(rec.meshes[0], tris)
    ctx.commit_deformed()
    got = ctx.render(B.camera(centre, radius), RES, RES, SPP, jit)[0]
    assert same(got, fresh_answers(contexts, 3, "blob(1025)", "twist")[0]["frame"])


@pytest.mark.gpu
def test_every_device_of_a_context_refits_its_copy(contexts):
    two = ft.Context(device=[0, 0])
    try:
        two.set_option("bvh_builder", 3)
        e = CAT["blob(1025)"]
        rec = Recorder(two)
        B.build_scene(rec, e.tris)
        tris, centre, radius = deform(e, "twist")
        two.set_mesh_triangles(rec.meshes[0], tris)
        two.commit_deformed()
        got = two.render(B.camera(centre, radius), RES, RES, SPP, ft.jitter_pattern(SPP))[0]
        assert same(got, fresh_answers(contexts, 3, "blob(1025)", "twist")[0]["frame"])
    finally:
        two.close()

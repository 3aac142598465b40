"""ft_scene_tree_quality and "refit_rebuild_percent" (Context.tree_quality): the measured surface-area cost of a mesh's tree
as it lies in device memory, and the rebuild in place that ft_scene_commit_deformed runs for an edited, device-built mesh once that cost has
grown past the host's threshold.  The cost is held against a numpy replay over Context.mesh_trees() (tests/refit_cost.py); a rebuilt tree is
held to the standard of every builder here - tests/bvh_tools.check_trees, every array bitwise the fresh context's, frames, surface planes and
ray queries bitwise those of a fresh context whose graph was built with the new vertices and committed with ft_scene_commit.

Deformations: those of tests/test_mesh_refit.py, plus `shuffle`: triangle i gets the vertices of triangle perm(i), the worst case for a tree
that keeps its topology.  Frames at 96x96x4 spp as there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import bvh_tools as B
from . import helpers as H
from . import test_mesh_refit as M
from .refit_cost import tree_cost
from .test_mesh_refit import Recorder, answers, assert_same_answers, assert_same_topology, same

CAT = B.catalogue()
MESHES = ["blob(65)", "blob(257)", "blob(1025)", "flat", "two_clusters", "identical"]
RES, SPP = M.RES, M.SPP
# The terms are non-negative, so any-order summation of the at most about 4100 terms here is off by under 5e-13 relative; 1e-10 leaves room
# for the order and still catches a single leaf missed or counted twice, each about 1e-5 of the total.
COST_RTOL = 1e-10
ARRAYS = ("nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes")


def shuffled(tris, seed=3):
    return np.ascontiguousarray(tris[np.random.default_rng(seed).permutation(tris.shape[0])])


def deform(e, how):
    if how == "shuffle":
        return shuffled(e.tris), e.centre, e.radius
    return M.deform(e, how)


def bits(x):
    return np.float64(x).view(np.uint64)


def options(ctx, builder, percent=0, pbl=1, lss=2):
    for k, v in (("bvh_builder", builder), ("primary_block_lists", pbl), ("light_space_shadows", lss), ("refit_rebuild_percent", percent)):
        ctx.set_option(k, v)


def close_to_replay(cost, T, what, mesh=0):
    want = tree_cost(T, mesh)
    print(f"{what}: cost {cost!r}, replay {want!r}")
    assert np.isfinite(cost) and cost > 0.0, what
    assert abs(cost - want) <= COST_RTOL * want, f"{what}: cost {cost!r} is not the replay's {want!r} (rel {abs(cost - want) / want:.3e})"


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


def fresh(get, builder, tris, view, key, pbl=1, lss=2):
    """A fresh graph of `tris` committed with ft_scene_commit: its answers, trees, the cost of its tree and what the commit reports; once per key."""
    key = (builder, pbl, lss) + tuple(key)
    if key not in _FRESH:
        ctx = get("fresh")
        options(ctx, builder, 0, pbl, lss)
        rec = Recorder(ctx)
        B.build_scene(rec, tris)
        _FRESH[key] = {"answers": answers(ctx, view, tris), "trees": ctx.mesh_trees(), "quality": ctx.tree_quality(rec.meshes[0]), "times": ctx.commit_times()}
    return _FRESH[key]


def fresh_of(get, builder, name, how, pbl=1, lss=2):
    tris, centre, radius = deform(CAT[name], how)
    return fresh(get, builder, tris, (centre, radius), (name, how), pbl, lss)


def committed(get, builder, name, percent=0, pbl=1, lss=2):
    """The work context with the catalogue mesh committed under the options: (ctx, mesh node, trees as built)."""
    ctx = get("work")
    options(ctx, builder, percent, pbl, lss)
    rec = Recorder(ctx)
    B.build_scene(rec, CAT[name].tris)
    return ctx, rec.meshes[0], ctx.mesh_trees()


def refit(ctx, node, e, how):
    tris, centre, radius = deform(e, how)
    ctx.set_mesh_triangles(node, tris)
    ctx.commit_deformed()
    return tris, (centre, radius)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_and_library_exports_the_quality_query():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert re.search(r"int32_t ft_scene_tree_quality\(ft_context\* ctx, ft_node mesh_node, double out\[4\]\);", hdr)
    assert '"refit_rebuild_percent"' in hdr
    lib = C.CDLL(ft.HIP_LIB)
    assert hasattr(lib, "ft_scene_tree_quality")
    doc = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\[<DllImport\(Lib\)>\] extern int ft_scene_tree_quality\(", doc)
    assert callable(ft.Context.tree_quality) and not hasattr(_capi.SceneBuilder, "tree_quality")


def test_refit_rebuild_percent_takes_zero_or_a_percentage_from_100():
    ctx = ft.Context(host_only=True)
    lib = ft.hip_lib()
    for v in (0, 100, 200, 1000000):
        assert lib.ft_set_option(ctx._ctx, b"refit_rebuild_percent", v) == 0, v
    for v in (-1, 1, 99, 1000001):
        assert lib.ft_set_option(ctx._ctx, b"refit_rebuild_percent", v) == -1, v
    ctx.close()


def test_tree_quality_errors_come_in_order_on_a_host_only_context():
    ctx = ft.Context(host_only=True)
    lib = ft.hip_lib()
    out = np.zeros(4)
    p = _capi.dptr(out)
    ctx.clear()
    hd = {"flat": ctx.bsp_mesh(0, CAT["blob(9)"].tris.reshape(-1, 9)), "deep": ctx.bsp_mesh(2, CAT["blob(63)"].tris.reshape(-1, 9)),
          "few": ctx.bsp_mesh(0, CAT["blob(7)"].tris.reshape(-1, 9)), "cube": ctx.primitive(ft.CUBE)}
    ctx.set_objects(ctx.group([hd["flat"], ctx.transform([("translate", (0, 3, 0))], hd["deep"]), ctx.transform([("translate", (0, -3, 0))], hd["few"]),
                               ctx.transform([("translate", (3, 0, 0))], hd["cube"])]))
    ctx.add_directional((0, -1, 1), (1, 1, 1))
    q = lib.ft_scene_tree_quality
    assert q(None, hd["flat"], p) == -1
    # before any commit: bad arguments are still FT_ERR_INVALID, a good mesh node is FT_ERR_STATE
    assert q(ctx._ctx, hd["flat"], None) == -1 and q(ctx._ctx, -1, p) == -1 and q(ctx._ctx, 10_000, p) == -1 and q(ctx._ctx, hd["cube"], p) == -1
    for k in ("flat", "deep", "few"):
        assert q(ctx._ctx, hd[k], p) == -5, k
    ctx.commit()
    assert q(ctx._ctx, hd["flat"], None) == -1 and q(ctx._ctx, -1, p) == -1 and q(ctx._ctx, 10_000, p) == -1 and q(ctx._ctx, hd["cube"], p) == -1
    assert q(ctx._ctx, hd["deep"], p) == -4 and q(ctx._ctx, hd["few"], p) == -4
    assert q(ctx._ctx, hd["flat"], p) == -2
    with pytest.raises(ft.FtError) as e:
        ctx.tree_quality(hd["flat"])
    assert e.value.status == -2
    assert not out.any()
    ctx.close()


def test_refit_rebuild_percent_is_not_a_commit_time_option():
    ctx = ft.Context(host_only=True)
    rec = Recorder(ctx)
    B.build_scene(rec, CAT["blob(65)"].tris)
    ctx.set_option("refit_rebuild_percent", 200)
    ctx.set_mesh_triangles(rec.meshes[0], shuffled(CAT["blob(65)"].tris))
    ctx.commit_deformed()                                            # FT_ERR_STATE if the option had asked for a full commit
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("builder", [0, 1, 3])
def test_cost_is_the_replays_and_cost_built_stays_through_refits(contexts, builder, name):
    ctx, node, T0 = committed(contexts, builder, name)
    q0 = ctx.tree_quality(node)
    assert bits(q0["cost"]) == bits(q0["cost_built"]) and q0["rebuilds"] == 0 and q0["rebuildable"] == (builder != 0), q0
    close_to_replay(q0["cost"], T0, f"builder {builder} {name} as built")
    for how in M.DEFORMS:
        refit(ctx, node, CAT[name], how)
        q = ctx.tree_quality(node)
        assert bits(q["cost_built"]) == bits(q0["cost_built"]) and q["rebuilds"] == 0, (how, q)
        close_to_replay(q["cost"], ctx.mesh_trees(), f"builder {builder} {name} {how} (ratio {q['ratio']:.3f})")


@pytest.mark.gpu
def test_cost_built_is_recorded_by_the_first_refit_when_no_query_came_earlier(contexts):
    ctx, node, T0 = committed(contexts, 3, "blob(257)")
    refit(ctx, node, CAT["blob(257)"], "twist")
    q = ctx.tree_quality(node)
    close_to_replay(q["cost_built"], T0, "cost_built after a refit, first asked for afterwards")
    close_to_replay(q["cost"], ctx.mesh_trees(), "cost after the refit")
    assert bits(q["cost"]) != bits(q["cost_built"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("builder", [1, 3])
def test_default_option_never_rebuilds(contexts, builder, name):
    ctx, node, T0 = committed(contexts, builder, name)
    tris, view = refit(ctx, node, CAT[name], "shuffle")
    q = ctx.tree_quality(node)
    print(f"builder {builder} {name} shuffle: cost ratio {q['ratio']:.3f}")
    assert q["rebuilds"] == 0 and q["rebuildable"] == 1
    assert_same_topology(T0, ctx.mesh_trees(), f"{name} shuffle")
    assert_same_answers(answers(ctx, view, tris), fresh_of(contexts, builder, name, "shuffle")["answers"], f"builder {builder} {name} shuffle")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["jitter", "far", "small"])
@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("builder", [1, 3])
def test_mild_deformations_stay_below_the_threshold_of_200(contexts, builder, name, how):
    ctx, node, T0 = committed(contexts, builder, name, percent=200)
    refit(ctx, node, CAT[name], how)
    q = ctx.tree_quality(node)
    print(f"builder {builder} {name} {how}: cost ratio {q['ratio']:.3f}")
    assert q["rebuilds"] == 0, q
    assert_same_topology(T0, ctx.mesh_trees(), f"{name} {how}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,pbl,lss", [("blob(257)", 1, 2), ("blob(1025)", 1, 2), ("flat", 1, 2), ("blob(257)", 0, 0)])
@pytest.mark.parametrize("builder", [1, 3])
def test_shuffle_rebuilds_in_place_into_the_fresh_contexts_tree(contexts, builder, name, pbl, lss):
    ctx, node, _ = committed(contexts, builder, name, percent=200, pbl=pbl, lss=lss)
    before = ctx.tree_quality(node)
    tris, view = refit(ctx, node, CAT[name], "shuffle")
    q, T = ctx.tree_quality(node), ctx.mesh_trees()
    F = fresh_of(contexts, builder, name, "shuffle", pbl, lss)
    print(f"builder {builder} {name}: cost as first built {before['cost_built']!r}, rebuilt {q['cost_built']!r}, fresh {F['quality']['cost']!r}")
    assert q["rebuilds"] == 1 and q["rebuildable"] == 1, q
    assert len(B.check_trees(T)) == 1
    assert bits(q["cost"]) == bits(q["cost_built"]) == bits(F["quality"]["cost"])
    for k in ARRAYS:                                                 # finds a range that was not reset
        assert same(T[k], F["trees"][k]), f"{k} is not the fresh context's"
    assert T["jobs"] == F["trees"]["jobs"]
    assert_same_answers(answers(ctx, view, tris), F["answers"], f"builder {builder} {name} shuffle, rebuilt, lists {pbl} light-space {lss}")


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [1, 3])
def test_identical_triangles_shuffled_do_not_rebuild_at_100(contexts, builder):
    """The shuffle of `identical` moves nothing.  Whether the refit tree's cost is then the built tree's to the last bit is measured first,
    with the option at 0; only if it is does a threshold of 100 have to leave the tree alone."""
    e = CAT["identical"]
    ctx, node, _ = committed(contexts, builder, "identical")
    refit(ctx, node, e, "shuffle")
    q = ctx.tree_quality(node)
    print(f"builder {builder} identical shuffle: cost {q['cost']!r}, cost_built {q['cost_built']!r}")
    ctx, node, T0 = committed(contexts, builder, "identical", percent=100)
    refit(ctx, node, e, "shuffle")
    r = ctx.tree_quality(node)
    print(f"builder {builder} identical shuffle at 100: rebuilds {r['rebuilds']}")
    if bits(q["cost"]) == bits(q["cost_built"]):
        assert r["rebuilds"] == 0
        assert_same_topology(T0, ctx.mesh_trees(), "identical shuffle")


@pytest.mark.gpu
def test_a_host_built_tree_is_measured_and_never_rebuilt(contexts):
    ctx, node, T0 = committed(contexts, 0, "blob(257)", percent=200)
    tris, view = refit(ctx, node, CAT["blob(257)"], "shuffle")
    q = ctx.tree_quality(node)
    print(f"builder 0 blob(257) shuffle: cost ratio {q['ratio']:.3f}")
    assert q["rebuildable"] == 0 and q["rebuilds"] == 0 and q["ratio"] > 2.0, q
    assert_same_topology(T0, ctx.mesh_trees(), "host-built")
    assert_same_answers(answers(ctx, view, tris), fresh_of(contexts, 0, "blob(257)", "shuffle")["answers"], "host-built, shuffled")


@pytest.mark.gpu
def test_refits_and_rebuilds_after_a_rebuild(contexts):
    e = CAT["blob(257)"]
    ctx, node, _ = committed(contexts, 3, "blob(257)", percent=200)
    first = ctx.tree_quality(node)["cost_built"]
    refit(ctx, node, e, "shuffle")
    q1, T1 = ctx.tree_quality(node), ctx.mesh_trees()
    assert q1["rebuilds"] == 1
    # a plain refit of the rebuilt tree
    moved = shuffled(e.tris) + np.random.default_rng(22).normal(size=e.tris.shape) * 0.01 * e.radius
    ctx.set_mesh_triangles(node, moved)
    ctx.commit_deformed()
    q2, T2 = ctx.tree_quality(node), ctx.mesh_trees()
    assert q2["rebuilds"] == 1 and bits(q2["cost_built"]) == bits(q1["cost_built"]), q2
    assert len(B.check_trees(T2)) == 1
    assert_same_topology(T1, T2, "the refit after the rebuild")
    close_to_replay(q2["cost"], T2, "cost of the refit after the rebuild")
    view = (e.centre, e.radius)
    assert_same_answers(answers(ctx, view, moved), fresh(contexts, 3, moved, view, ("blob(257)", "shuffle+jitter"))["answers"], "the refit after the rebuild")
    # a second, different permutation
    again = shuffled(moved, seed=4)                                  # (of the jittered vertices: a set of triangles the first tree was not built for)
    ctx.set_mesh_triangles(node, again)
    ctx.commit_deformed()
    q3 = ctx.tree_quality(node)
    assert q3["rebuilds"] == 2 and bits(q3["cost"]) == bits(q3["cost_built"]), q3
    assert len(B.check_trees(ctx.mesh_trees())) == 1
    assert_same_answers(answers(ctx, view, again), fresh(contexts, 3, again, view, ("blob(257)", "shuffle4"))["answers"], "the second rebuild")
    # a full commit starts over
    ctx.commit()
    q4 = ctx.tree_quality(node)
    assert q4["rebuilds"] == 0 and bits(q4["cost"]) == bits(q4["cost_built"]) == bits(q3["cost_built"]), q4
    close_to_replay(q4["cost_built"], ctx.mesh_trees(), "cost_built after the full commit")
    assert bits(q4["cost_built"]) != bits(first)


@pytest.mark.gpu
def test_a_taller_rebuilt_tree_gets_its_stack(contexts):
    ctx = contexts("work")
    options(ctx, 1, 100)
    rec = Recorder(ctx)
    B.build_scene(rec, B.blob(287))
    T0, h0 = ctx.mesh_trees(), ctx.commit_times()["device_bvh_height"]
    tall = CAT["chain(256)"]
    assert tall.tris.shape[0] == 287
    ctx.set_mesh_triangles(rec.meshes[0], tall.tris)
    ctx.commit_deformed()
    q, T = ctx.tree_quality(rec.meshes[0]), ctx.mesh_trees()
    view = (tall.centre, tall.radius)
    F = fresh(contexts, 1, tall.tris, view, ("chain(256)", "as is"))
    print(f"blob(287) -> chain(256): height {h0} -> {ctx.commit_times()['device_bvh_height']} (fresh {F['times']['device_bvh_height']}), "
          f"stacks {T0['stack_capacity']} -> {T['stack_capacity']} (fresh {F['trees']['stack_capacity']})")
    assert q["rebuilds"] == 1, q
    assert F["trees"]["stack_capacity"] > T0["stack_capacity"], "the case does not make a taller tree"
    assert T["stack_capacity"] == F["trees"]["stack_capacity"]
    assert ctx.commit_times()["device_bvh_height"] >= F["times"]["device_bvh_height"]
    assert len(B.check_trees(T)) == 1
    for k in ARRAYS:
        assert same(T[k], F["trees"][k]), f"{k} is not the fresh context's"
    assert_same_answers(answers(ctx, view, tall.tris), F["answers"], "the taller rebuilt tree")


@pytest.mark.gpu
def test_temporal_accumulation_survives_a_rebuild_in_place(contexts):
    """The sequence of test_temporal_accumulation_survives_commit_deformed, with a shuffle between two accumulates."""
    W, Hh, calls = 96, 64, 6
    e = CAT["blob(257)"]
    jit = np.zeros((1, 2))
    cams = [B.camera(e.centre + np.array([0.05 * k, 0.0, 0.0]), 2.0 * e.radius) for k in range(calls)]

    def run(ctx, percent):
        options(ctx, 3, percent)
        m = M._ground_scene(ctx, e.tris)
        ctx.temporal_begin(W, Hh)
        out = []
        for k, cam in enumerate(cams):
            if k == 3:
                ctx.set_mesh_triangles(m, shuffled(e.tris))
                ctx.commit_deformed()
            ctx.render(cam, W, Hh, 1, jit, seed=100 + k, fetch=False)
            ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
            out.append((ctx.temporal_fetch(), ctx.temporal_status()))
        ctx.temporal_end()
        return out, ctx.tree_quality(m)["rebuilds"]

    plain, n0 = run(contexts("fresh"), 0)
    rebuilt, n1 = run(contexts("work"), 200)
    assert (n0, n1) == (0, 1)
    for k, ((f0, s0), (f1, s1)) in enumerate(zip(plain, rebuilt)):
        assert s0 == s1 and s0["calls"] == k + 1, k
        assert all(same(x, y) for x, y in zip(f0, f1)), f"call {k}: M, Q or N differ from the sequence that only refits"


def _pair_scene(b, tris_a, tris_b):
    b.clear()
    a, c = b.bsp_mesh(0, tris_a.reshape(-1, 9)), b.bsp_mesh(0, tris_b.reshape(-1, 9))
    b.set_objects(b.group([b.transform([("translate", (-2.0, 0.0, 0.0))], b.material(a, colour=(0.9, 0.5, 0.2))),
                           b.transform([("translate", (2.0, 0.0, 0.0))], b.material(c, colour=(0.3, 0.6, 0.9)))]))
    b.add_directional((1, -2, 1), (1, 1, 1))
    b.commit()
    return a, c


@pytest.mark.gpu
def test_a_rebuild_leaves_the_other_meshes_of_the_scene_alone(contexts):
    ctx, other = contexts("work"), contexts("fresh")
    for c in (ctx, other):
        options(c, 3, 200)
    ea, eb = CAT["blob(257)"], CAT["blob(1025)"]
    a, b = _pair_scene(ctx, ea.tris, eb.tris)
    T0, qb0 = ctx.mesh_trees(), ctx.tree_quality(b)
    new_a, new_b = shuffled(ea.tris), M.deform(eb, "jitter")[0]
    ctx.set_mesh_triangles(a, new_a)
    ctx.set_mesh_triangles(b, new_b)
    ctx.commit_deformed()
    qa, qb, T1 = ctx.tree_quality(a), ctx.tree_quality(b), ctx.mesh_trees()
    assert qa["rebuilds"] == 1 and qb["rebuilds"] == 0 and bits(qb["cost_built"]) == bits(qb0["cost_built"]), (qa, qb)
    assert [r["n"] for r in B.check_trees(T1)] == [257, 1025]
    jb = [j for j in T1["jobs"] if j["n"] == 1025][0]
    spans = {"nodes": (jb["node_base"], jb["n"] - 1), "bsp_leaves": (jb["leaf_base"], 2 * jb["n"] - 1), "tri_orig": (jb["tri_base"], jb["n"]), "tri_src": (jb["tri_base"], jb["n"])}
    for k, (f, n) in spans.items():
        if k == "nodes":
            for field in ("left", "right", "axis"):
                assert np.array_equal(T0[k][field][f:f + n], T1[k][field][f:f + n]), f"the jittered mesh's {k}.{field} changed"
        else:
            assert np.array_equal(T0[k][f:f + n], T1[k][f:f + n]), f"the jittered mesh's {k} changed"
    wf = jb["wide_base"]
    assert np.array_equal(B._wide_children(T0)[wf:wf + jb["n"] - 1], B._wide_children(T1)[wf:wf + jb["n"] - 1]), "the jittered mesh's 4-wide children changed"
    close_to_replay(qb["cost"], T1, "the jittered mesh", mesh=1)
    close_to_replay(qa["cost"], T1, "the rebuilt mesh", mesh=0)
    cam, jit = B.camera(np.zeros(3), 4.0), ft.jitter_pattern(SPP)
    _pair_scene(other, new_a, new_b)
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], other.render(cam, RES, RES, SPP, jit)[0])
    # the rebuilt mesh's ranges are the fresh context's; the jittered mesh keeps the old vertices' tree
    F1 = other.mesh_trees()
    ja = [j for j in T1["jobs"] if j["n"] == 257][0]
    for k, f, n in (("nodes", ja["node_base"], 256), ("bsp_leaves", ja["leaf_base"], 513), ("tris", ja["tri_base"], 257), ("tri_orig", ja["tri_base"], 257), ("wide", ja["wide_base"], 256)):
        assert same(T1[k][f:f + n], F1[k][f:f + n]), f"the rebuilt mesh's {k} are not the fresh context's"
    assert same(T1["meshes"], F1["meshes"]) and T1["jobs"] == F1["jobs"]


@pytest.mark.gpu
def test_every_device_of_a_context_rebuilds_its_copy(contexts):
    e = CAT["blob(1025)"]
    one = contexts("work")
    two = ft.Context(device=[0, 0])
    try:
        frames = []
        for ctx in (one, two):
            options(ctx, 3, 200)
            rec = Recorder(ctx)
            B.build_scene(rec, e.tris)
            tris, view = refit(ctx, rec.meshes[0], e, "shuffle")
            assert ctx.tree_quality(rec.meshes[0])["rebuilds"] == 1
            frames.append(ctx.render(B.camera(*view), RES, RES, SPP, ft.jitter_pattern(SPP))[0])
        assert same(frames[0], frames[1]), "the two-device frame is not the single-device context's"
        assert same(frames[0], fresh_of(contexts, 3, "blob(1025)", "shuffle")["answers"]["frame"])
    finally:
        two.close()

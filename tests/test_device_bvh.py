"""The device BVH builders (ft_bvh.hip: the linear BVH, "bvh_builder" = 1, and the binned surface-area tree, 3) on degenerate meshes
and at their limits.  The trees are read back from HBM (Context.mesh_trees) and walked by tests/bvh_tools.check_trees BEFORE any ray
is traced through them; then rays, frames and the triangle plane are compared with the host builder's (0) bit for bit and with the
oracle's brute force.

Measured on an MI355X (reported device_bvh_height / height of the emitted tree): chain(256) linear 38 / 36, surface-area 13 / 13;
chain(1024) linear 40 / 38 (accepted, at the limit), surface-area 15 / 15; chain(2048) linear 41 (refused: the host's tree, 34),
surface-area 16 / 16; geometric linear 10 / 8, surface-area 33 / 33.  DESIGN.md 15 holds the table."""
import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import bvh_tools as B
from . import helpers as H

CAT = B.catalogue()
NAMES = list(CAT)
RES = 96
N_RAYS = 20000
TIE_MESHES = ("identical", "concentric", "chain(256)", "chain(1024)", "chain(2048)")     # step 5: the triangle plane


# ---------------------------------------------------------------------------------------------------------------- references, once
_ORACLE = {}


def _oracle_of(key, build, centre, radius, tris):
    """The oracle's answers for one scene, computed once per session and never modified."""
    if key not in _ORACLE:
        orc = O.Oracle()
        build(orc)
        o, d, md = B.rays_for((centre, radius), tris, n=N_RAYS)
        cam = B.camera(centre, radius)
        frame, _ = orc.render(cam, RES, RES, 1, np.zeros((1, 2)))
        ans = {"rays": (o, d, md), "closest": orc.closest(o, d), "blocked": orc.blocked(o, d, md), "cam": cam, "frame": frame}
        ys, xs = np.mgrid[0:RES, 0:RES]                              # the rays through the pixel centres, for the triangle plane
        po, pd = np.zeros((RES * RES, 3)), np.zeros((RES * RES, 3))
        for k, (x, y) in enumerate(zip(xs.ravel(), ys.ravel())):
            po[k], pd[k] = O.ray_through_pixel(cam, RES, RES, int(x), int(y))
        hit, t, *_ = orc.closest(po, pd)
        ans["pixels"] = (po, pd, hit.astype(bool), t)
        orc.close()
        _ORACLE[key] = ans
    return _ORACLE[key]


def _oracle_mesh(name):
    e = CAT[name]
    return _oracle_of(name, lambda b: B.build_scene(b, e.tris), e.centre, e.radius, e.tris)


# ---------------------------------------------------------------------------------------------------------------- not GPU
def test_catalogue_is_deterministic_finite_and_off_the_cell_borders():
    again = B.make_catalogue()
    assert list(again) == NAMES and len(NAMES) == len(B.BLOB_SIZES) + 11
    for name, e in CAT.items():
        assert np.array_equal(e.tris, again[name].tris) and e.exact == again[name].exact, name
        assert np.isfinite(e.tris).all() and e.tris.shape[1:] == (3, 3) and e.tris.shape[0] <= 2100, name
        assert B.key_margin(e.tris, e.exact) >= 1e-6, f"{name}: a box centre within 1e-6 of a Morton cell border"
    assert [CAT[f"chain({d})"].tris.shape[0] for d in (256, 1024, 2048)] == [287, 1055, 2079]
    assert (CAT["flat"].tris[:, :, 2] == 0.37).all() and (CAT["flat_x"].tris[:, :, 0] == 0.37).all()
    e = CAT["two_clusters"]
    q = np.unique(B.morton_keys(e.tris))
    assert q.tolist() == [0, 0x3FFFFFFF], "each cluster in one Morton cell"
    assert np.unique(B.morton_keys(CAT["identical"].tris)).size == 1 and np.unique(B.morton_keys(CAT["concentric"].tris)).size == 1
    d = CAT["degenerate"].tris
    area = np.linalg.norm(np.cross(d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]), axis=1)
    assert int((area < 1e-12).sum()) == 100


def test_replay_gives_the_chain_heights():
    """The radix tree peels one of the 30 key bits per level and then halves the d equal keys by position: 30 + log2(d)."""
    for d, total, height in ((256, 287, 38), (1024, 1055, 40), (2048, 2079, 41)):
        keys, order, fit, walked = B.replay_linear(CAT[f"chain({d})"].tris)
        assert keys.shape[0] == total and fit == height and walked == height - 2, (d, fit, walked)
        assert np.array_equal(order[:d], np.arange(d)), "equal keys stay in list order"


@pytest.fixture(scope="module")
def host_trees():
    """name -> read-back of a host-only context (the host builder's trees), once."""
    out = {}
    ctx = ft.Context(host_only=True)
    for name, e in CAT.items():
        B.build_scene(ctx, e.tris)
        out[name] = ctx.mesh_trees()
    B.build_multi(ctx, CAT["chain(2048)"].tris)
    out["multi"] = ctx.mesh_trees()
    ctx.close()
    return out


def test_host_only_context_commits_every_mesh_and_its_trees_pass_the_checker(host_trees):
    for name, T in host_trees.items():
        assert not T["from_device"] and T["jobs"] == []
        reports = B.check_trees(T)
        if name == "multi":
            assert [r["n"] for r in reports] == [8, 257, 1025, 2079]    # blob(7) has no BVH, the bspMesh 3 is a real BSP
        elif name == "blob(7)":
            assert reports == []
        else:
            assert len(reports) == 1 and reports[0]["n"] == CAT[name].tris.shape[0] and not reports[0]["device_built"], name


def test_oracle_answers_closest_on_every_mesh():
    for name, e in CAT.items():
        orc = O.Oracle()
        B.build_scene(orc, e.tris)
        o, d, _ = B.rays_for((e.centre, e.radius), e.tris, n=2000)
        hit, t, p, n, _ = orc.closest(o, d)
        m = hit.astype(bool)
        assert m.any() and not m.all(), name
        assert np.isfinite(t[m]).all() and np.isfinite(p[m]).all() and np.isfinite(n[m]).all(), name
        orc.close()


def _copy(T):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in T.items()}


def test_checker_fails_on_corrupted_trees(host_trees):
    good = host_trees["blob(257)"]
    rep = B.check_trees(good)[0]
    # a box one ulp below the highest vertex under it
    bad = _copy(good)
    node = int(good["nodes"]["left"][rep["bvh_root"]])
    assert node >= 0
    bad["nodes"]["bmax"][node, 1] = np.nextafter(rep["need"][node][1][1], -np.inf)
    with pytest.raises(AssertionError, match="does not hold what is below it"):
        B.check_trees(bad)
    # the same through the 4-wide tree alone: the slot boxes are copies
    bad = _copy(good)
    w = int(good["meshes"][rep["mesh"], 3])
    bad["wide"][w, 3] = np.nextafter(bad["wide"][w, 3], -np.inf) - 1.0
    with pytest.raises(AssertionError, match="slot 0 of wide node"):
        B.check_trees(bad)
    # two tri_orig entries swapped against their records
    bad = _copy(good)
    f = int(good["bsp_leaves"][~rep["leaf_refs"][0]][0])
    bad["tri_orig"][[f, f + 1]] = bad["tri_orig"][[f + 1, f]]
    with pytest.raises(AssertionError, match="not its tri_orig's record"):
        B.check_trees(bad)
    # a leaf range dropped
    bad = _copy(good)
    bad["bsp_leaves"][~rep["leaf_refs"][3]] = (0, 0)
    with pytest.raises(AssertionError, match="is empty"):
        B.check_trees(bad)
    bad = _copy(good)                                               # ... or replaced by a copy of its neighbour
    bad["bsp_leaves"][~rep["leaf_refs"][3]] = bad["bsp_leaves"][~rep["leaf_refs"][4]]
    with pytest.raises(AssertionError):
        B.check_trees(bad)
    # a coarse box removed
    first, count = (int(x) for x in good["meshes"][rep["mesh"], 4:6])
    failures = 0
    for k in range(first, first + count):
        bad = _copy(good)
        bad["coarse_boxes"][k] = np.nan
        try:
            B.check_trees(bad)
        except AssertionError as e:
            assert "no coarse box holds" in str(e)
            failures += 1
    assert failures >= count // 2, f"removing a coarse box went unnoticed for {count - failures} of {count}"
    bad = _copy(good)                                               # the count cut short
    bad["meshes"][rep["mesh"], 5] = count - 1
    with pytest.raises(AssertionError, match="no coarse box holds"):
        B.check_trees(bad)
    # a tree too tall for the stacks it reports
    bad = _copy(good)
    bad["stack_capacity"] = rep["height"]
    with pytest.raises(AssertionError, match="does not fit the per-lane stacks"):
        B.check_trees(bad)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _triangle_plane_check(tris, orc_ans, plane, what):
    """The `triangle` plane against a brute force over the pixel rays: on every pixel the oracle hits, the named triangle is hit at the
    oracle's t, and among coincident copies of it the lowest list index is named (BspMesh.fs:95-97 scans in list order)."""
    o, d, m, t = orc_ans["pixels"]
    got = plane.ravel()
    assert np.array_equal(got >= 0, m), f"{what}: the triangle plane's hit pixels are not the oracle's"
    if not m.any():
        return 0
    rec = np.ascontiguousarray(np.concatenate([tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]], axis=1))
    _, inverse = np.unique(rec.view(np.dtype((np.void, 72))).ravel(), return_inverse=True)
    lowest = np.full(inverse.max() + 1, tris.shape[0])
    np.minimum.at(lowest, inverse, np.arange(tris.shape[0]))
    g = got[m]
    assert (lowest[inverse[g]] == g).all(), f"{what}: a coincident hit did not go to the lowest list index"
    v0, e1, e2 = rec[g, 0:3], rec[g, 3:6], rec[g, 6:9]               # Moeller-Trumbore on the named triangle
    pv = np.cross(d[m], e2)
    inv = 1.0 / np.einsum("ij,ij->i", e1, pv)
    tv = o[m] - v0
    u = np.einsum("ij,ij->i", tv, pv) * inv
    qv = np.cross(tv, e1)
    v = np.einsum("ij,ij->i", d[m], qv) * inv
    tt = np.einsum("ij,ij->i", e2, qv) * inv
    tol = 1e-9
    assert (u >= -tol).all() and (v >= -tol).all() and (u + v <= 1 + tol).all(), f"{what}: a pixel names a triangle its ray misses"
    assert np.max(np.abs(tt - t[m]) / (1.0 + np.abs(t[m]))) <= tol, f"{what}: a pixel names a triangle that is not the closest"
    return int(m.sum())


def _one_pass(hip, build, builder, ans, expect_device, replay_of=None, what=""):
    """Commit under `builder`, check the read-back tree BEFORE any ray walks it, then trace: (closest, blocked, frame, trees, commit times)."""
    hip.set_option("bvh_builder", builder)
    build(hip)                                                      # the commit returns OK, also where the device builder refuses
    ct = hip.commit_times()
    T = hip.mesh_trees()
    assert T["from_device"]
    height = ct["device_bvh_height"]
    assert (height > 0) == expect_device and (len(T["jobs"]) > 0) == expect_device, f"{what}: device_bvh_height {height}, {len(T['jobs'])} jobs"
    replays = {j["mesh"]: replay_of(j["mesh"]) for j in T["jobs"]} if (replay_of and builder == 1) else None
    reports = B.check_trees(T, device_bvh_height=height if expect_device else None, replays=replays)
    print(f"HEIGHTS {what} builder {builder}: reported {height}, walked {[r['height'] for r in reports]}, 4-wide depth {[r['wide_depth'] for r in reports]}, stacks {T['stack_capacity']}")
    o, d, md = ans["rays"]
    closest, blocked = hip.closest(o, d), hip.blocked(o, d, md)
    jit = np.zeros((1, 2))
    frame, st = hip.render(ans["cam"], RES, RES, 1, jit)
    hip.set_option("classify_pixels", 0)
    try:
        plain, _ = hip.render(ans["cam"], RES, RES, 1, jit)
    finally:
        hip.set_option("classify_pixels", 1)
    assert np.array_equal(plain, frame), f"{what}: pixel classification changed the frame"
    print(f"CULLED {what} builder {builder}: {st['rays_primary_culled']} of {st['rays_primary']}")
    assert st["rays_primary_culled"] > 0, f"{what}: the corners of the frame see background, yet no block was culled"
    return {"closest": closest, "blocked": blocked, "frame": frame, "trees": T, "height": height, "reports": reports}


def _compare(ref, got, ans, what):
    for x, y in zip(ref["closest"], got["closest"]):
        assert np.array_equal(x, y), f"{what}: closest differs from builder 0's"
    assert np.array_equal(ref["blocked"], got["blocked"]), f"{what}: blocked differs from builder 0's"
    assert np.array_equal(ref["frame"], got["frame"]), f"{what}: frame differs from builder 0's"
    H.assert_hits_match(got["closest"], ans["closest"], what=what)
    assert np.array_equal(got["blocked"], ans["blocked"]), f"{what}: blocked differs from the oracle's"
    assert H.assert_frames_match(got["frame"], ans["frame"], what=what) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_builders_on_the_catalogue(hip, name):
    """Every catalogue mesh under the host builder (0), the linear BVH (1) and the surface-area tree (3).  blob(7) is below the device's
    eight triangles; chain(2048) under the linear builder is one level too tall (41): the device refuses it, the commit returns OK with
    the host's tree in HBM; chain(1024) is accepted at exactly 40."""
    e = CAT[name]
    ans = _oracle_mesh(name)
    replay = B.replay_linear(e.tris)
    res = {}
    try:
        for builder in (0, 1, 3):
            on_device = builder != 0 and name != "blob(7)" and not (name == "chain(2048)" and builder == 1)
            res[builder] = _one_pass(hip, lambda b: B.build_scene(b, e.tris), builder, ans, on_device, replay_of=lambda m: replay, what=f"{name}")
            if name in TIE_MESHES:
                plane = hip.render_aov(ans["cam"], RES, RES, 1, np.zeros((1, 2)), channels=["triangle"])["triangle"]
                res[builder]["hits"] = _triangle_plane_check(e.tris, ans, plane, f"{name}, builder {builder}")
    finally:
        hip.set_option("bvh_builder", 2)
    H.assert_hits_match(res[0]["closest"], ans["closest"], what=f"{name}, builder 0")
    for builder in (1, 3):
        _compare(res[0], res[builder], ans, f"{name}, builder {builder}")
    assert int(ans["closest"][0].sum()) > 100, "the rays must hit the mesh"
    if name in TIE_MESHES:
        assert res[0]["hits"] > 0, "the camera must see the mesh"
    if name == "chain(1024)":
        assert res[1]["height"] == 40 and res[1]["reports"][0]["height"] == 38
    if name == "chain(256)":
        assert res[1]["height"] == 38
    if name == "chain(2048)":
        assert res[1]["height"] == 0 and not res[1]["reports"][0]["device_built"]     # the host's tree, read back from HBM
        for k in ("nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes"):
            assert res[1]["trees"][k].tobytes() == res[0]["trees"][k].tobytes(), f"{k}: not the host builder's"
    if name in ("geometric", "chain(2048)"):
        assert 0 < res[3]["height"] <= 40


def _multi_oracle(key, extra):
    return _oracle_of(key, lambda b: B.build_multi(b, extra), *B.MULTI_VIEW, None)


def _multi_replay(m):
    names = [n for n, _, _ in B.MULTI_PARTS] + ["chain(2048)"]
    return B.replay_linear(CAT[names[m]].tris)


@pytest.mark.gpu
def test_several_device_built_meshes_in_one_scene(hip):
    """blob(8), blob(257), blob(1025) under transforms around a sphere, with a blob(7) and a bspMesh 3: three jobs whose ranges all
    start past zero.  Under 1 and 3 every job passes the checker and everything matches builder 0 and the oracle; under 2 (by size)
    nothing goes to the device.  (The recommit: test_recommitting_the_same_graph_gives_the_same_trees.)"""
    ans = _multi_oracle("multi", None)
    res = {}
    try:
        for builder in (0, 1, 3, 2):
            res[builder] = _one_pass(hip, lambda b: B.build_multi(b), builder, ans, builder in (1, 3), replay_of=_multi_replay, what="multi")
            if builder in (1, 3):
                T = res[builder]["trees"]
                assert [j["n"] for j in T["jobs"]] == [8, 257, 1025]
                for j in T["jobs"][1:]:                              # every range of the later jobs starts past zero
                    assert min(j[k] for k in ("first_global", "node_base", "leaf_base", "tri_base", "wide_base", "coarse_first")) > 0, j
    finally:
        hip.set_option("bvh_builder", 2)
    H.assert_hits_match(res[0]["closest"], ans["closest"], what="multi, builder 0")
    for builder in (1, 3, 2):
        _compare(res[0], res[builder], ans, f"multi, builder {builder}")
    assert int(ans["closest"][0].sum()) > 1000


@pytest.mark.gpu
def test_one_refused_mesh_sends_the_whole_scene_to_the_host_builder(hip):
    """multi with chain(2048) as a fourth mesh under the linear builder: its tree is 41 levels tall, the device refuses it, and the
    commit falls back to the host builder once, for the whole scene - no job remains, and every mesh still matches the oracle."""
    extra = CAT["chain(2048)"].tris
    ans = _multi_oracle("multi+chain", extra)
    res = {}
    try:
        for builder in (0, 1):
            res[builder] = _one_pass(hip, lambda b: B.build_multi(b, extra), builder, ans, False, what="multi + chain(2048)")
        assert [r["n"] for r in res[1]["reports"]] == [8, 257, 1025, 2079] and not any(r["device_built"] for r in res[1]["reports"])
        res[3] = _one_pass(hip, lambda b: B.build_multi(b, extra), 3, ans, True, what="multi + chain(2048)")
        assert [j["n"] for j in res[3]["trees"]["jobs"]] == [8, 257, 1025, 2079]
    finally:
        hip.set_option("bvh_builder", 2)
    for builder in (1, 3):
        _compare(res[0], res[builder], ans, f"multi + chain(2048), builder {builder}")


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [1, 2, 3])
def test_recommitting_the_same_graph_gives_the_same_trees(hip, builder):
    """Committing the multi scene twice leaves bitwise the same arrays in HBM.  (The surface-area builder once numbered the children
    of a level with an atomic counter, in the order its waves happened to run: `nodes`, `bsp_leaves` and `wide` then differed from commit
    to commit.  k_sah_assign numbers them by a scan over the level's open nodes.)"""
    keys = ("nodes", "bsp_leaves", "tris", "tri_orig", "tri_src", "wide", "coarse_boxes", "meshes")
    try:
        hip.set_option("bvh_builder", builder)
        B.build_multi(hip)
        first = hip.mesh_trees()
        B.check_trees(first, device_bvh_height=hip.commit_times()["device_bvh_height"] or None)
        hip.commit()
        again = hip.mesh_trees()
    finally:
        hip.set_option("bvh_builder", 2)
    assert (len(first["jobs"]) == 3) == (builder != 2)
    differ = [k for k in keys if first[k].tobytes() != again[k].tobytes()]
    print(f"RECOMMIT builder {builder}: arrays that differ {differ}")
    assert not differ, f"builder {builder}: {differ} differ after a recommit of the same graph"
    assert first["jobs"] == again["jobs"] and first["stack_capacity"] == again["stack_capacity"]

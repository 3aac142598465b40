"""The light-space shadow tree and grid (ft_scene.cpp, build_light_space; ft_kernels.hip, mesh_shadow_packet / mesh_shadow_grid) on the
hard-mesh catalogue of tests/bvh_tools.py, each mesh a shadow CASTER over a receiver (tests/shadow_tools.py).

The CPU half proves on a host-only context and the oracle what each case exercises: the structures the host builder makes hold what they
must (check_tree, check_grid) and are of the expected kind (no pairs under 8 triangles, a tree alone where a cell would overflow, cells of
more than 64 and 128 entries, grids one cell wide); the walk's stack cannot overflow; the mesh's shadow lies on the receiver, and on the
mesh itself where it can; and the waves of the frame reach the grid route, the tree route behind it, full cells and border cells.

The GPU half renders every case at 1 and 4 samples and asserts, per frame: the options light_space_shadows 0, 1, 2 give the same bits and
counters; shadow rays were traced; the oracle's frame within helpers.PIXEL_RTOL; and the per-lane BVH walk (coherent_waves = 0) bit for
bit."""
import numpy as np
import pytest

import functracer_amd as ft

from . import helpers as H
from . import shadow_tools as S
from . import walk_tools as W
from .test_light_space_grid import check_grid, grid_of, render_three
from .test_light_space_shadows import NONE, check_tree, pair_root

gpu = pytest.mark.gpu
NAMES = list(S.CASES)
MODULE_LIGHTS = sorted({tuple(float(x) for x in l[1]) for c in S.CASES.values() for l in c.lights if l[0] == "dir"})


def _mesh_of(name):
    return S.CASES[name].parts[0][0]


# =============================================================================================================================
# CPU half

def test_every_mesh_and_kind_of_light_of_the_plan_is_covered():
    assert {_mesh_of(n) for n in S.SINGLE} == set(S.MESHES)
    for mesh in S.MESHES:
        lights = {tuple(float(x) for x in l[1]) for n in S.SINGLE if _mesh_of(n) == mesh for l in S.CASES[n].lights}
        assert len(lights) >= 2, mesh
    for n, c in S.CASES.items():
        assert c.w <= 96 and c.h <= 72
    assert sum(c.tiles is not None for c in S.CASES.values()) == 1


@pytest.mark.parametrize("name", NAMES)
def test_structures_hold_and_are_what_the_case_claims(name):
    """check_tree and check_grid for every pair of every caster; and the kind of structure each mesh is in the plan for."""
    case = S.CASES[name]
    pairs, nodes, ls_tris, leaf_pairs = S.structures(name)
    assert leaf_pairs[len(case.parts)] == 0xFFFFFFFF, "the receiver is no mesh"
    for part, (mesh, ops, kind) in enumerate(case.parts):
        n = len(S.mesh_tris(mesh))
        recs = S.pairs_of(name, part)
        if n < 8 or kind == "unlit":
            assert recs == [], (mesh, kind)
            continue
        assert len(recs) == len(S.dir_lights(case))
        base = int(leaf_pairs[part])
        for l, light in enumerate(case.lights):                     # point and soft lights have neither tree nor grid
            if light[0] != "dir":
                assert pair_root(pairs[base + l]) == NONE and grid_of(pairs[base + l])[2] == 0
        for l, rec in recs:
            what = f"{name} part {part} light {l}"
            assert pair_root(rec) >= 0, what
            frame = np.array([rec[0:3], rec[3:6], rec[6:9]])
            assert np.allclose(frame @ frame.T, np.eye(3), atol=1e-14), what
            assert check_tree(rec, nodes, ls_tris) == n, what
            _, s, nu, nv = grid_of(rec)
            if mesh in S.TREE_ONLY:
                assert nu == 0, what
                continue
            assert nu > 0, f"{what}: no grid"
            check_grid(rec, nodes, ls_tris, n)
            counts = S.cell_counts(rec, nodes)
            print(f"{what}: grid {nu} x {nv}, fullest cell {counts.max()}, {(counts > 64).sum()} cells over 64, {(counts == 0).sum()} empty")
            if mesh == "concentric":
                assert (counts > 128).any(), what
            if mesh == "geometric":
                assert (counts > 64).sum() >= 1, what
                assert (counts == 0).any(), what


def test_flat_meshes_lit_in_their_plane_get_grids_one_cell_wide():
    for name, light in (("flat-in-plane", 1), ("flat_x-in-plane", 1)):
        recs = dict(S.pairs_of(name))
        _, _, nu, nv = grid_of(recs[light])
        assert min(nu, nv) == 1 and max(nu, nv) >= 64, (name, nu, nv)
    for name in ("flat-off-plane", "flat_x-off-plane"):             # 1e-3 off the plane: still one cell wide
        _, _, nu, nv = grid_of(dict(S.pairs_of(name))[1])
        assert min(nu, nv) == 1 and max(nu, nv) >= 64, (name, nu, nv)


@pytest.mark.parametrize("mesh", S.TREE_ONLY)
def test_crowded_meshes_keep_the_tree_alone_under_every_light_of_the_module(mesh):
    """A cell would hold more than kLsGridMaxCell entries: identical and the chains' 256 and 2048 equal triangles, the clusters' 400.
    One exception, kept as a case of its own: along the diagonal the two clusters project onto each other, the spot they fill is the
    whole (u, v) extent, and the 800 triangles get a grid like any blob."""
    pairs, nodes, ls_tris, leaf_pairs = S.mesh_structures(mesh, MODULE_LIGHTS)
    n = len(S.mesh_tris(mesh))
    for l in range(len(MODULE_LIGHTS)):
        rec = pairs[int(leaf_pairs[0]) + l]
        assert pair_root(rec) >= 0
        assert S.worst_stack(rec, nodes) <= S.WAVE_STACK
        if mesh == "two_clusters" and MODULE_LIGHTS[l] == tuple(float(x) for x in S.DIAGONAL):
            check_grid(rec, nodes, ls_tris, n)
            continue
        assert grid_of(rec)[2] == 0, (mesh, MODULE_LIGHTS[l])
        if mesh != "chain(2048)" or l == 0:                          # (the box check is quadratic in Python: once for the largest)
            assert check_tree(rec, nodes, ls_tris) == n


def test_blob_of_seven_triangles_gets_no_pairs_and_eight_do():
    assert S.pairs_of("blob(7)") == [] and len(S.pairs_of("blob(8)")) == 2


@pytest.mark.parametrize("name", NAMES)
def test_tree_walk_stack_holds_every_tree(name):
    """ls_tree_walk keeps its pending children in a WaveStack of 64 entries and checks no overflow: with EVERY child entered, the trees of
    the cases stay far below."""
    _, nodes, _, _ = S.structures(name)
    for part in range(len(S.CASES[name].parts)):
        for l, rec in S.pairs_of(name, part):
            worst = S.worst_stack(rec, nodes)
            print(f"{name} part {part} light {l}: worst stack {worst}")
            assert worst <= S.WAVE_STACK


def test_tree_walk_stack_holds_a_mesh_built_for_depth():
    """deep(4096): every binned level peels the few largest triangles, so the tree is as tall as the builder lets a mesh of its size
    become; and the bound the builder implies at kLsMaxTris triangles."""
    n = len(S.mesh_tris("deep(4096)"))
    assert n >= 4096
    lights = [S.GENERAL, (0.0, 0.0, 1.0), S.HAIR, S.DIAGONAL]
    pairs, nodes, ls_tris, leaf_pairs = S.mesh_structures("deep(4096)", lights)
    bound, levels = S.stack_bound(n)
    worst = []
    for l in range(len(lights)):
        rec = pairs[int(leaf_pairs[0]) + l]
        assert pair_root(rec) >= 0
        worst.append(S.worst_stack(rec, nodes))
        assert worst[-1] <= bound <= S.WAVE_STACK
    print(f"deep(4096): worst stack {worst}, bound for {n} triangles {bound} ({levels} binary levels)")
    assert max(worst) >= 30, "the mesh is not deep"
    assert check_tree(pairs[int(leaf_pairs[0])], nodes, ls_tris) == n
    assert S.stack_bound(S.LS_MAX_TRIS) == (51, 34)                 # 16 binned + 18 median levels, 17 wide nodes, 3 pushes each
    assert S.stack_bound(S.LS_MAX_TRIS)[0] <= S.WAVE_STACK


@pytest.mark.parametrize("name", NAMES)
def test_shadows_exist_on_the_oracle(name):
    S.assert_shadows_exist(name)


@pytest.mark.parametrize("name", [n for n in S.SINGLE if _mesh_of(n) not in S.TREE_ONLY and _mesh_of(n) != "blob(7)" and S.CASES[n].tiles is None])
def test_both_routes_are_reached(name):
    S.assert_routes_reached(name)


def test_two_lights_cast_shadows_on_disjoint_parts_of_the_receiver():
    a, b = S.shadow_masks("two-lights-apart").values()
    print(f"two-lights-apart: {a.sum()} and {b.sum()} receiver pixels shadowed, {(a & b).sum()} by both")
    assert a.sum() >= 50 and b.sum() >= 50 and (a ^ b).sum() >= 50
    assert (a & b).sum() == 0, "the shadows overlap"


def test_multi_leaf_scene_has_bases_and_offsets_other_than_zero():
    case = S.CASES["multi-leaf"]
    pairs, _, _, leaf_pairs = S.structures("multi-leaf")
    assert [l[0] for l in case.lights] == ["soft", "point", "dir", "dir"]
    assert [p[0] for p in case.parts] == ["blob(8)", "blob(7)", "blob(65)", "blob(65)"] and case.parts[2][2] == "unlit" and case.parts[3][2] == "same"
    assert leaf_pairs[0] == 0 and leaf_pairs[1] == 0xFFFFFFFF and leaf_pairs[2] == 0xFFFFFFFF
    assert leaf_pairs[3] == len(case.lights)                        # one record per light, directional or not
    assert [l for l, _ in S.dir_lights(case)] == [2, 3]
    for part in (0, 3):
        assert [pair_root(pairs[int(leaf_pairs[part]) + l]) != NONE for l in range(4)] == [False, False, True, True]


# =============================================================================================================================
# GPU half

# A context of the module's own (as tests/test_coherent_walks.py): the tests switch coherent_waves and the commit-time light_space_shadows.
@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("spp", (1, 4))
@pytest.mark.parametrize("name", NAMES)
def test_hard_casters_on_the_device(ctx, name, spp):
    S.assert_shadows_exist(name)                                    # on the CPU, before anything runs
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    cam, jit = W.camera(view), S.jitter(spp)
    what = f"{name} x{spp}"
    frame, st = render_three(ctx, lambda c: S.build(c, case), cam, view.w, view.h, spp, jitter=jit, tiles=view.tiles)
    assert st["rays_shadow"] > 0, what
    assert not np.isnan(frame).any(), what
    worst = H.assert_frames_match(frame, S.reference_frame(name, spp), what=what)
    print(f"{what}: {st['rays_shadow']} shadow rays, worst pixel against the oracle {worst:.3e}")
    S.build(ctx, case)                                              # (render_three's last set_option left the scene to be committed again)
    ctx.set_option("coherent_waves", 0)
    try:
        per_lane, _ = ctx.render(cam, view.w, view.h, spp, jit, tiles=view.tiles)
    finally:
        ctx.set_option("coherent_waves", 1)
    diff = np.any(frame != per_lane, axis=2)
    assert not diff.any(), f"{what}: the per-lane BVH walk differs on {int(diff.sum())} pixels, first {np.argwhere(diff)[:3].tolist()}"

"""Option "deform_light_space" (include/functracer_hip.h "deforming meshes"): ft_scene_commit_deformed refits the
light-space shadow trees of the meshes it edits and builds their grids again on the device instead of stripping them.

The CPU half: the option exists, the header names it, and a host-only deformed commit under it is the fresh host commit byte for byte.
(tools/deform_ls_host_check.cpp checks the flattener's ls_src and the host derivation of c, R and s_abs under ASan + UBSan as a
stand-alone program; its build line is in its first comment.)

The GPU half sets the option to 1, deforms the casters of the shadow cases (tests/shadow_tools.py) with the deformations of
tests/test_mesh_refit.py and compares, after every call, with a second context built from scratch with the new vertices: the pair
records' doubles [0..13] bit for bit, the tree (it passes check_tree, and its leaf records are the new records as a multiset), the grid
(the same resolution and the same cells - entry boxes, records, order) and frames and counters at 1 and 4 samples.  Then the sequences
with ft_scene_commit_lights, other casters, two leaves over one mesh, option 0 before option 1, R past 2e29, the temporal accumulation,
the rebuild in place, temporal_follow_deformed, a queued frame and two devices."""
import functools
import math
import os

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd._capi import FtError

from . import bvh_tools as B
from . import helpers as H
from . import light_tools as L
from . import shadow_tools as S
from . import walk_tools as W
from .test_light_space_grid import check_grid, grid_cells, grid_of
from .test_light_space_shadows import check_tree, light_space, pair_root
from .test_mesh_refit import DEFORMS, deform

gpu = pytest.mark.gpu
STRIPPED = 0xFFFFFFFF
NO_TREE = -(1 << 31)
NAMES = ("blob(8)", "blob(65)-xf", "blob(65)-mirror", "concentric", "two_clusters", "identical", "chain(256)", "multi-leaf")
EDITED = {"multi-leaf": ("blob(8)", "blob(65)")}                   # the meshes a case's deformation edits; default: its only one


def edited_meshes(name):
    return EDITED.get(name, (S.CASES[name].parts[0][0],))


@functools.lru_cache(maxsize=None)
def moved(mesh, how, amount=1.0):
    t = np.ascontiguousarray(deform(B.catalogue()[mesh], how, amount)[0].reshape(-1, 9))
    t.setflags(write=False)
    return t


def new_vertices(name, how, amount=1.0):
    return {mesh: moved(mesh, how, amount) for mesh in edited_meshes(name)}


def build(b, case, lights, tris_of=None):
    """light_tools.build with other vertices for the meshes `tris_of` names; returns {catalogue name: mesh node}."""
    tris_of = tris_of or {}
    recv_ops, _ = S.geometry(case)
    b.clear()
    items, node, handles = [], None, {}
    for mesh, ops, kind in case.parts:
        if kind != "same":
            node = b.bsp_mesh(0, tris_of.get(mesh, S.mesh_tris(mesh).reshape(-1, 9)))
            handles[mesh] = node
        item = b.material(b.transform(list(ops), node) if ops else node, colour=S.MESH_COLOUR)
        items.append(b.ignore_light(item) if kind == "unlit" else item)
    items.append(b.material(b.transform(recv_ops, b.primitive(ft.SQUARE)), colour=S.RECEIVER_COLOUR))
    b.set_objects(b.group(items))
    L.add_lights(b, lights)
    b.commit()
    return handles


def deform_to(ctx, handles, tris_of):
    for mesh, t in tris_of.items():
        ctx.set_mesh_triangles(handles[mesh], t)
    ctx.commit_deformed()


def records_of(tris9):
    """The records (v0, v1 - v0, v2 - v0) of vertices (a, b, c), as the flattener and k_refit_records form them."""
    t = np.asarray(tris9, dtype=np.float64).reshape(-1, 3, 3)
    return np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], axis=1)


def tree_records(rec, nodes, ls_tris):
    """The leaf records of a pair's tree, in the order a walk finds them."""
    out, stack = [], [pair_root(rec)]
    while stack:
        n = stack.pop()
        for ch in nodes[n, 20:24].view(np.int32).tolist():
            if ch == NO_TREE:
                continue
            if ch >= 0:
                stack.append(ch)
            else:
                out.extend(ls_tris[((~ch) >> 3) + k] for k in range((~ch) & 7))
    return out


def tree_nodes(rec, nodes):
    out, stack = [], [pair_root(rec)]
    while stack:
        n = stack.pop()
        out.append(n)
        stack.extend(ch for ch in nodes[n, 20:24].view(np.int32).tolist() if ch >= 0)
    return sorted(out)


def _cells_bytes(cells):
    return {key: [(b.tobytes(), t.tobytes()) for b, t in entries] for key, entries in cells.items()}


def render(c, view, spp, **kw):
    return c.render(W.camera(view), view.w, view.h, spp, S.jitter(spp), tiles=view.tiles, **kw)


def same_frames(ctx, fresh, view, what, shadows=True):
    first = None
    for spp in (1, 4):
        a, sa = render(ctx, view, spp)
        b, sb = render(fresh, view, spp)
        diff = np.any(a != b, axis=2) & ~(np.isnan(a).all(axis=2) & np.isnan(b).all(axis=2))
        assert not diff.any(), f"{what} x{spp}: {int(diff.sum())} pixels differ from the fresh context, first {np.argwhere(diff)[:3].tolist()}"
        assert L.counters(sa) == L.counters(sb), f"{what} x{spp}"
        assert not shadows or sa["rays_shadow"] > 0, what
        first = a if first is None else first
    return first


def same_queries(ctx, fresh, view, lights, what):
    o, d, _, _ = W.pixel_rays(view)
    ha, hb = ctx.closest(o, d), fresh.closest(o, d)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ha, hb)), what
    v = np.asarray(next(l[1] for l in lights if l[0] == "dir"), dtype=np.float64)
    hit = ha[0].astype(bool)
    origin = (ha[2] + S.SLIGHT_OFFSET * ha[3])[hit]
    back = np.broadcast_to(-v, origin.shape).copy()
    far = np.full(len(origin), 1e300)
    assert np.array_equal(ctx.blocked(origin, back, far), fresh.blocked(origin, back, far)), what
    ga = ctx.render_aov(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
    gb = fresh.render_aov(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
    planes = [key for key in gb if isinstance(gb[key], np.ndarray)]
    assert len(planes) >= 8 and all(ga[key].tobytes() == gb[key].tobytes() for key in planes), what


def same_structures(ctx, fresh, case, lights, tris_of, what, stripped=()):
    """Every pair of every lit caster of `ctx` against the fresh context's.  Returns {(part, light): (n_u, n_v)} of the pairs with a tree."""
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    fpairs, fnodes, fls_tris, fleaf_pairs = light_space(fresh)
    kinds = {}
    for part, (mesh, ops, kind) in enumerate(case.parts):
        tris = tris_of.get(mesh, S.mesh_tris(mesh).reshape(-1, 9))
        n = len(tris)
        base, fbase = int(leaf_pairs[part]), int(fleaf_pairs[part])
        if n < 8 or kind == "unlit" or part in stripped:
            assert base == STRIPPED, (what, part)
            continue
        assert base != STRIPPED and fbase != STRIPPED, f"{what}: leaf {part} lost its pairs"
        want = sorted(r.tobytes() for r in records_of(tris))
        for l, light in enumerate(lights):
            rec, frec = pairs[base + l], fpairs[fbase + l]
            label = f"{what} part {part} light {l}"
            assert rec[:14].tobytes() == frec[:14].tobytes(), f"{label}: pair doubles [0..13] are not the fresh commit's"
            assert (pair_root(rec) >= 0) == (pair_root(frec) >= 0), label
            if pair_root(frec) < 0:
                assert pair_root(rec) == NO_TREE and grid_of(rec)[2] == 0, label
                continue
            assert check_tree(rec, nodes, ls_tris) == n, label
            assert sorted(t.tobytes() for t in tree_records(rec, nodes, ls_tris)) == want, f"{label}: the tree's leaf records are not the new records"
            (_, s, nu, nv), (_, fs, fnu, fnv) = grid_of(rec), grid_of(frec)
            assert (s, nu, nv) == (fs, fnu, fnv), f"{label}: grid {(s, nu, nv)}, the fresh context's {(fs, fnu, fnv)}"
            kinds[(part, l)] = (nu, nv)
            if nu == 0:
                continue
            cells = check_grid(rec, nodes, ls_tris, n)
            assert _cells_bytes(cells) == _cells_bytes(grid_cells(frec, fnodes, fls_tris)), f"{label}: the grid's cells are not the fresh commit's"
            assert L.attempt_rule(L._entry_boxes(cells), n) == (s, nu, nv), label
    return kinds


def arrays(ctx):
    return [a.tobytes() for a in light_space(ctx)[:3]]


# =============================================================================================================================
# CPU half

def test_the_option_is_accepted_and_any_value_means_one():
    ctx = ft.Context(host_only=True)
    for v in (1, 0, 7, -3, 0):
        ctx.set_option("deform_light_space", v)
    with pytest.raises(FtError) as e:
        ctx.set_option("deform_light_spaces", 1)
    assert "unknown option" in str(e.value)
    ctx.close()


def test_the_header_names_the_option():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    comment = hdr[:hdr.index("int32_t ft_set_option(")]
    assert '"deform_light_space" (0 = default; any other value means 1' in comment[comment.rindex("/*"):]
    paragraph = hdr[:hdr.index("int32_t ft_scene_commit_deformed(")]
    paragraph = paragraph[paragraph.rindex("/*"):]
    assert 'ft_set_option("deform_light_space", 1)' in paragraph and "256 MiB" in paragraph
    assert ft.hip_lib().ft_abi_version() == 2 and "#define FT_ABI_VERSION 2" in hdr


@pytest.mark.parametrize("how", DEFORMS)
def test_host_only_commit_deformed_under_the_option_is_the_fresh_host_commit(how):
    for name in ("blob(65)-xf", "multi-leaf"):
        case = S.CASES[name]
        lights = L.initial(case)
        ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)
        ctx.set_option("deform_light_space", 1)
        handles = build(ctx, case, lights)
        tris_of = new_vertices(name, how)
        deform_to(ctx, handles, tris_of)
        build(fresh, case, lights, tris_of)
        assert [a.tobytes() for a in light_space(ctx)] == [a.tobytes() for a in light_space(fresh)], (name, how)
        ctx.close()
        fresh.close()


# =============================================================================================================================
# GPU half

@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    c.set_option("deform_light_space", 1)
    yield c
    c.set_option("light_space_shadows", 2)
    c.close()


@pytest.fixture(scope="module")
def fresh():
    c = ft.Context(device=0)
    yield c
    c.close()


def _options(ctx, fresh, **opts):
    defaults = {"light_space_shadows": 2, "bvh_builder": 2, "refit_rebuild_percent": 0, "temporal_follow_deformed": 0}
    defaults.update(opts)
    for k, v in defaults.items():
        ctx.set_option(k, v)
        if k in ("light_space_shadows", "bvh_builder"):
            fresh.set_option(k, v)
    ctx.set_option("deform_light_space", 1)


@gpu
@pytest.mark.parametrize("lss", (1, 2))
@pytest.mark.parametrize("how", DEFORMS)
@pytest.mark.parametrize("name", NAMES)
def test_a_deformed_caster_keeps_its_structures_and_gives_the_fresh_contexts_results(ctx, fresh, name, how, lss):
    _options(ctx, fresh, light_space_shadows=lss)
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    before, _ = render(ctx, view, 1)
    tris_of = new_vertices(name, how)
    deform_to(ctx, handles, tris_of)
    build(fresh, case, lights, tris_of)
    what = f"{name} {how} option {lss}"
    leaf_pairs = light_space(ctx)[3]
    for part, (mesh, _, kind) in enumerate(case.parts):
        if mesh in tris_of and kind != "unlit" and len(tris_of[mesh]) >= 8:
            assert leaf_pairs[part] != STRIPPED, f"{what}: the edited leaf {part} was stripped"
    kinds = same_structures(ctx, fresh, case, lights, tris_of, what)
    print(f"{what}: grids {kinds}")
    assert kinds and (lss == 2 or all(nu == 0 for nu, _ in kinds.values()))
    frame = same_frames(ctx, fresh, view, what)
    if how == "twist":
        assert not np.array_equal(frame, before, equal_nan=True), f"{what}: the frame did not change"
        same_queries(ctx, fresh, view, lights, what)


@gpu
def test_deformations_and_turning_lights_in_turn(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    base = L.initial(case)
    tilted = [("dir", L.tilt(l[1], math.radians(15.0)), l[2]) for l in base]
    A, Bv = new_vertices(name, "jitter"), new_vertices(name, "twist")
    handles = build(ctx, case, base)
    full = light_space(ctx)
    steps = [("deform to A", A, base), ("tilted by 15 degrees", A, tilted), ("deform to B", Bv, tilted), ("the full commit's direction again", Bv, base)]
    tris_now, lights_now = None, base
    for what, tris_of, lights in steps:
        if tris_of is not tris_now:
            deform_to(ctx, handles, tris_of)
        if lights is not lights_now:
            L.set_lights(ctx, lights)
            ctx.commit_lights()
        tris_now, lights_now = tris_of, lights
        build(fresh, case, lights, tris_of)
        kinds = same_structures(ctx, fresh, case, lights, tris_of, what)
        assert all(nu > 0 for nu, _ in kinds.values()), (what, kinds)
        same_frames(ctx, fresh, view, what)
    # step 4 did not bring the full commit's record or grid back (same_structures has compared both with the fresh context's; and plainly:)
    pairs, _, _, leaf_pairs = light_space(ctx)
    first = int(leaf_pairs[0])
    assert first == int(full[3][0])
    assert all(pairs[first + l].tobytes() != full[0][first + l].tobytes() for l in range(len(base)))
    assert all(grid_of(pairs[first + l])[0] >= full[1].size for l in range(len(base))), "a deformed pair's grid lies in the full commit's arrays"
    # A, B, A, B: the second visit leaves the bytes and the sizes of the first
    kept = {}
    for turn in range(2):
        for key, tris_of in (("A", A), ("B", Bv)):
            deform_to(ctx, handles, tris_of)
            got = arrays(ctx)
            assert kept.setdefault(key, got) == got, f"visit {turn + 1} of {key} left other bytes or sizes"


def _footprint(rec, nodes, ls_tris):
    """Every byte one pair owns: its record, its tree's nodes and leaf records, its grid's cells."""
    own = [rec.tobytes(), nodes[tree_nodes(rec, nodes)].tobytes()] + [t.tobytes() for t in tree_records(rec, nodes, ls_tris)]
    if grid_of(rec)[2]:
        own.append(sorted(_cells_bytes(grid_cells(rec, nodes, ls_tris)).items()))
    return own


@gpu
def test_the_other_caster_of_the_scene_keeps_every_byte(ctx, fresh):
    _options(ctx, fresh)
    case, view = S.CASES["multi-leaf"], S.view_of(S.CASES["multi-leaf"])
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    dirs = [l for l, light in enumerate(lights) if light[0] == "dir"]

    def other():
        pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
        return [_footprint(pairs[int(leaf_pairs[3]) + l], nodes, ls_tris) for l in dirs]
    before = other()
    assert all(grid_of(light_space(ctx)[0][int(light_space(ctx)[3][3]) + l])[2] > 0 for l in dirs)
    tris_of = {"blob(8)": moved("blob(8)", "twist")}
    deform_to(ctx, handles, tris_of)
    assert other() == before
    build(fresh, case, lights, tris_of)
    same_structures(ctx, fresh, case, lights, tris_of, "one of two casters")
    same_frames(ctx, fresh, view, "one of two casters")


@gpu
def test_one_mesh_node_under_two_transforms_has_both_leaves_refit(ctx, fresh):
    _options(ctx, fresh)
    far = [("rotate", (0.0, 1.0, 0.0), 0.9), ("scale", (2.5, 3.0, 2.2)), ("translate", (0.5, 0.3, 2.5))]
    parts = [("blob(65)", [("translate", (0.0, 0.0, -2.5))], "lit"), ("blob(65)", far, "same")]
    case = S.Case("two-leaves", parts, S.CASES["multi-leaf"].lights, S.Cam(300, 70, 0.4, 45, 0.5), (1.0, 16.0), 96, 72, None, None)
    view = S.view_of(case)
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    tris_of = {"blob(65)": moved("blob(65)", "jitter", 3.0)}
    deform_to(ctx, handles, tris_of)
    build(fresh, case, lights, tris_of)
    kinds = same_structures(ctx, fresh, case, lights, tris_of, "two leaves")
    assert {part for part, _ in kinds} == {0, 1}
    same_frames(ctx, fresh, view, "two leaves")


@gpu
def test_a_leaf_stripped_with_the_option_off_stays_stripped(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    ctx.set_option("deform_light_space", 0)
    deform_to(ctx, handles, new_vertices(name, "jitter"))
    assert light_space(ctx)[3][0] == STRIPPED
    ctx.set_option("deform_light_space", 1)
    tris_of = new_vertices(name, "twist")
    deform_to(ctx, handles, tris_of)
    assert light_space(ctx)[3][0] == STRIPPED
    build(fresh, case, lights, tris_of)
    same_structures(ctx, fresh, case, lights, tris_of, "stripped before", stripped=(0,))
    same_frames(ctx, fresh, view, "stripped before")
    ctx.commit()                                                    # the next full commit brings the structures back
    assert light_space(ctx)[3][0] != STRIPPED


@gpu
def test_a_mesh_too_large_for_a_tree_loses_it_and_gets_it_back(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    huge = {"blob(65)": np.ascontiguousarray(S.mesh_tris("blob(65)").reshape(-1, 9) * 1e30)}
    deform_to(ctx, handles, huge)
    pairs, _, _, leaf_pairs = light_space(ctx)
    assert leaf_pairs[0] != STRIPPED
    for l in range(len(lights)):
        assert pair_root(pairs[int(leaf_pairs[0]) + l]) == NO_TREE and grid_of(pairs[int(leaf_pairs[0]) + l])[2] == 0
    build(fresh, case, lights, huge)
    same_frames(ctx, fresh, view, "R past 2e29", shadows=False)
    back = new_vertices(name, "jitter")
    deform_to(ctx, handles, back)
    build(fresh, case, lights, back)
    kinds = same_structures(ctx, fresh, case, lights, back, "R back")
    assert kinds and all(nu > 0 for nu, _ in kinds.values())
    same_frames(ctx, fresh, view, "R back")


@gpu
def test_the_temporal_accumulation_stays_open(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    handles = build(ctx, case, L.initial(case))
    cam, jit = W.camera(view), S.jitter(1)
    ctx.temporal_begin(view.w, view.h)
    for k in range(3):
        if k == 2:
            deform_to(ctx, handles, new_vertices(name, "jitter"))
            assert light_space(ctx)[3][0] != STRIPPED
        ctx.render(cam, view.w, view.h, 1, jit, seed=100 + k, fetch=False)
        ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
        status = ctx.temporal_status()
        assert status["calls"] == k + 1
    assert status["with_history"] > 0
    ctx.temporal_end()


@gpu
def test_a_rebuild_in_place_keeps_the_light_space_structures(ctx, fresh):
    _options(ctx, fresh, bvh_builder=3, refit_rebuild_percent=100)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    tris_of = {"blob(65)": np.ascontiguousarray(moved("blob(65)", "jitter")[::-1])}   # every triangle where another one was
    deform_to(ctx, handles, tris_of)
    assert ctx.tree_quality(handles["blob(65)"])["rebuilds"] == 1
    build(fresh, case, lights, tris_of)
    kinds = same_structures(ctx, fresh, case, lights, tris_of, "rebuilt in place")
    assert kinds and all(nu > 0 for nu, _ in kinds.values())
    same_frames(ctx, fresh, view, "rebuilt in place")


@gpu
def test_temporal_follow_deformed_gives_what_it_gives_with_the_option_off(ctx, fresh):
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    cam, jit = W.camera(view), S.jitter(1)

    def run(option):
        _options(ctx, fresh, temporal_follow_deformed=1)
        ctx.set_option("deform_light_space", option)
        handles = build(ctx, case, L.initial(case))
        ctx.temporal_begin(view.w, view.h)
        out = []
        for k in range(4):
            if k >= 2:
                deform_to(ctx, handles, new_vertices(name, "jitter", float(k)))
            ctx.render(cam, view.w, view.h, 1, jit, seed=100 + k, fetch=False)
            ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
            out.append(([np.asarray(a).tobytes() for a in ctx.temporal_fetch()], ctx.temporal_status()))
        ctx.temporal_end()
        return out
    off, on = run(0), run(1)
    assert off == on and on[-1][1]["calls"] == 4 and on[-1][1]["with_history"] > 0
    ctx.set_option("deform_light_space", 1)


@gpu
def test_a_frame_queued_before_the_call_shows_the_old_mesh(ctx, fresh):
    _options(ctx, fresh)
    name = "blob(65)-xf"
    case, view = S.CASES[name], S.view_of(S.CASES[name])
    lights = L.initial(case)
    handles = build(ctx, case, lights)
    old, _ = render(ctx, view, 1)
    ctx.render_enqueue(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
    tris_of = new_vertices(name, "twist")
    deform_to(ctx, handles, tris_of)                                # retires the queued frame first
    assert np.array_equal(ctx.fetch_frame(np.zeros((view.h, view.w, 3))), old)
    build(fresh, case, lights, tris_of)
    new = same_frames(ctx, fresh, view, "after a queued frame")
    assert not np.array_equal(new, old)


def _two_devices(two, fresh):
    try:
        two.set_option("deform_light_space", 1)
        name = "multi-leaf"
        case, view = S.CASES[name], S.view_of(S.CASES[name])
        lights = L.initial(case)
        handles = build(two, case, lights)
        fresh.set_option("light_space_shadows", 2)
        fresh.set_option("bvh_builder", 2)
        for how in ("jitter", "twist"):
            tris_of = new_vertices(name, how)
            deform_to(two, handles, tris_of)
            build(fresh, case, lights, tris_of)
            same_structures(two, fresh, case, lights, tris_of, f"{two.devices()} {how}")
            for spp in (1, 4):
                a, sa = render(two, view, spp)
                b, _ = render(fresh, view, spp)
                assert np.array_equal(a, b, equal_nan=True), f"{two.devices()} {how} x{spp}"
                assert sa["rays_shadow"] > 0
    finally:
        two.close()


@gpu
def test_two_devices(fresh):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _two_devices(ft.Context(device=[0, 1]), fresh)


@gpu
def test_two_device_context_on_one_gpu(fresh):
    _two_devices(ft.Context(device=[0, 0]), fresh)

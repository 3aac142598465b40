"""The parallel-ray rule through every item cull and the block classifier.

A ray with |den| < 1e-7 against a flat face hits it at its own origin, any distance from the item (Plane.fs:13-16; plane_t), so every
cull in front of the exact intersection carries an exemption driven by the scene's face-direction table: item_missed_by (OP_CULL and
the sparse route of exact_cull), par_lane in exact_cull, rows_nearly_parallel in bundle_cull and bundle_cull_to_light, par_rows in
k_classify.  Random frames never produce such a den; here every ray is built to have one (tests/parallel_tools.py), in five bands
around the rule and around the culls' doubled threshold, against plane, square, circle, cube and solidCylinder under identity,
rotation, non-uniform scales of 1e-3 and 1e3, a shear, a mirror and nested transforms, bare and as either operand of subtract and
intersect (every target under every transform), on an item with 9
directions (no OP_CULL) and in a scene with 36 (no direction table).  One group of tests per site:

  1. explicit rays through Context.closest / blocked: thousands in one call (the float verdicts of exact_cull; with the target alone,
     plain OP_CULL) and about a hundred of the same rays again in calls of at most 8 (the sparse route) - up to 48 origin hits past
     the sphere, 16 near it and every thirty-second ray of the rest: thousands of rays eight at a time would be thousands of calls;
  2. primary rays of frames in which a whole pixel row (a band of rows at |row| = 1e-3) is parallel to a face: render_aov planes against
     the oracle's closest, the frame against the oracle's, classify_pixels x coherent_waves bitwise equal;
  3. shadow rays parallel to a face of a distant occluder, for a directional and a point light;
  4. reflected rays parallel to a face, at max_depth 2 and 8.

The first half needs no GPU: it proves on a host-only context, numpy and the oracle that every case is what it claims - the bands, the
oracle's hits at the origin exactly where the rule puts them, and that the item's bounding sphere alone would have dropped them.

Where the last proof cannot be had, the CPU half proves that instead.  The plane has no bounding sphere (its item is unbounded and never
culled).  The circle and the caps of the solidCylinder clip a hit at |p - centre| < 1 with p the ray's ORIGIN (Cylinder.fs:22): every
origin that can hit them lies inside the item's bounding sphere unless the transform stretches that unit ball past the sphere, which
among the transforms here only `tall` does.  Under CSG, operand B's hits outside a closed A are never kept (Csg.fs:27-44), so B's origin
hits all lie inside the item's bounds; and an open A (square, circle) lets B's box widen the item, so under `target & S`, whose S has
to hold the origins for the hits to survive, nothing is left outside it.  test_csg_cases_on_the_oracle asserts each of these, and a
minimum number of origin hits for every CSG case."""
import functools

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from . import parallel_tools as P

gpu = pytest.mark.gpu
BARE_CASES = [(prim, xf) for prim in P.TARGETS for xf in P.TRANSFORMS]
CSG_CASES = [(prim, xf, st) for prim in P.TARGETS for xf in P.TRANSFORMS for st in P.STRUCTURES[1:]]
FRAME_CASES = [(prim, xf, kind) for prim, xf in P.FRAME_CASES for kind in P.FRAME_KINDS]
PLANES = ["t", "p", "n", "colour", "leaf", "node"]


FACE_CLIP = {prim: faces[0].clip for prim, faces in P.FACES.items()}


def _cullable(prim, xf):
    """Can an origin hit lie outside the item's bounding sphere at all?  (The module docstring says why not.)"""
    return prim != "plane" and (FACE_CLIP[prim] != "ball" or xf == "tall")


# =============================================================================================================================
# CPU half

@pytest.mark.parametrize("prim,xf", BARE_CASES)
def test_rays_fall_into_the_den_bands(prim, xf):
    """From leaf_matrices() of a host-only context: the target's matrices are the numpy product of its transform list; every ray's
    row . d lies in its band; a ray built for one row of the cube is an ordinary ray (|den| >= 1e-5) for the other two; every origin
    stands at least 1e-3 model units off every face of its row; the scene holds what it should."""
    ref = P.reference(prim, xf, "bare")
    info, rays, W = ref["info"], ref["rays"], ref["w2m"][0]
    m, t = P.matrix(P.flat_ops(xf))
    assert np.allclose(ref["m2w"][0][:, :3], m, rtol=1e-12, atol=1e-15) and np.allclose(ref["m2w"][0][:, 3], t, rtol=1e-12, atol=1e-15)
    assert np.allclose(W[:, :3] @ m, np.eye(3), atol=1e-9)
    unbounded = prim == "plane"
    assert (info["items"], info["bounded_items"], info["unbounded"]) == (4, 3 if unbounded else 4, int(unbounded))
    assert info["face_directions"] == (0 if unbounded else len({f.row for f in P.FACES[prim]})), "an unbounded item is never culled: its direction is not tabled"
    assert len(rays.o) >= 500
    for row in sorted(set(rays.row.tolist())):
        R = W[row, :3]
        sel = rays.row == row
        den = rays.d[sel] @ R
        tol = 1e-15 * np.linalg.norm(R) * np.linalg.norm(rays.d[sel], axis=1).max()            # what another order of the same products can move
        assert np.abs(den - rays.den[sel]).max() <= 10 * tol
        assert (np.einsum("ij,ij->i", rays.d[sel], rays.d[sel]) > 1e-2).all()
        for band, (lo, hi) in P.BANDS.items():
            b = np.abs(den[rays.band[sel] == band])
            assert len(b) and (b >= lo).all() and (b <= hi).all(), (band, b.min(), b.max())
            if band != "zero":
                assert min(abs(b.min() - lo), abs(hi - b.max())) > 100 * tol
        for band in ("half", "cull", "near", "far"):
            assert {1.0, -1.0} <= set(np.sign(den[rays.band[sel] == band]).tolist()), f"{band}: both signs of den"
        for other in set(f.row for f in P.FACES[prim]) - {row}:
            assert (np.abs(rays.d[sel] @ W[other, :3]) >= 1e-5).all()
        model = rays.o[sel] @ W[:, :3].T + W[:, 3]
        assert np.allclose(model, rays.model[sel], rtol=1e-9, atol=1e-9)
        for f in P.FACES[prim]:
            if f.row == row:
                assert (np.abs(rays.model[sel][:, row] - f.offset) >= 1e-3 - 1e-12).all()
        above = np.array([P.origin_hit_expected(prim, row, p) for p in rays.model[sel]])
        assert above.any() and (~above).any(), "origins on both sides of the faces / of their clips"


@pytest.mark.parametrize("prim,xf", BARE_CASES)
def test_oracle_hits_at_the_origin_exactly_where_the_rule_says(prim, xf):
    """Every ray of the two parallel bands whose origin is on or above a face of its row and inside that face's clip comes back with
    t == 0 on the target and p == its origin; no other ray does; no control is ever hit at t == 0; and such a ray is blocked."""
    ref = P.reference(prim, xf, "bare")
    rays, (hit, t, p, _, col) = ref["rays"], ref["closest"]
    at_origin = P.origin_hits(ref)
    assert np.array_equal(at_origin, rays.expected), np.nonzero(at_origin != rays.expected)[0][:5]
    assert not at_origin[~np.isin(rays.band, P.PARALLEL_BANDS)].any()
    assert (np.abs(p[at_origin] - rays.o[at_origin]) <= H.TIGHT * (1.0 + np.abs(rays.o[at_origin]))).all()       # (p comes back through the transforms)
    assert at_origin.sum() >= 100
    leaf = P.leaf_of_colour(col, hit)
    assert ((hit != 0) == (leaf >= 0)).all()
    assert not ((leaf >= 10) & (t == 0.0)).any(), "a control hit at the origin"
    assert (leaf >= 10).sum() >= 2, "the controls stand in the rays' way"
    assert (ref["blocked"][at_origin] == 1).all()
    assert 0 < ref["blocked"].sum() < len(rays.o)


@pytest.mark.parametrize("prim,xf", BARE_CASES)
def test_the_bounding_sphere_alone_would_drop_the_origin_hits(prim, xf):
    """The sphere is recomputed as Flattener::end_item does.  At least a third of the origin hits, and at least 32, belong to rays whose
    line passes it at more than two radii; those rays come first and fill whole waves.  For the cases in which no origin hit can lie
    outside the sphere, that is what is shown."""
    ref = P.reference(prim, xf, "bare")
    rays, sphere, at_origin = ref["rays"], ref["sphere"], P.origin_hits(ref)
    if prim == "plane":
        assert sphere is None and ref["info"]["unbounded"] == 1
        return
    centre, radius = sphere
    if not _cullable(prim, xf):
        assert (np.linalg.norm(rays.o[rays.expected] - centre, axis=1) < radius).all()
        return
    far = P.line_distance(rays.o, rays.d, centre) > 2.0 * radius
    assert np.array_equal(far, rays.far)
    n = int((far & at_origin).sum())
    assert n >= 32 and 3 * n >= int(at_origin.sum()), (n, int(at_origin.sum()))
    assert ref["n_far"] >= 64 and ref["n_far"] % 64 == 0 and far[:ref["n_far"]].all()
    assert (at_origin[:ref["n_far"]].reshape(-1, 64).sum(axis=1) > 0).sum() >= 1, "a whole wave of far rays holds an origin hit"


@pytest.mark.parametrize("prim,xf,structure", CSG_CASES)
def test_csg_cases_on_the_oracle(prim, xf, structure):
    """Under subtract / intersect an origin hit appears only where the bare target has one, never in a non-parallel band, and the scene
    tables the target's directions whichever operand it is (none for an item the plane leaves unbounded).  Every case holds origin hits:
      intA  all of the bare target's (B holds every origin);
      subA  at least 32;
      as operand A, wherever an origin hit can lie outside the ITEM's bounding sphere at all, at least 32 of them belong to rays whose
            line passes that sphere at more than two radii.  The item's sphere is the target's own under a closed A (cube,
            solidCylinder); under an open A (square, circle) B's box counts too: the small sphere of subA is added here, and the sphere
            of intA, which holds every origin, leaves nothing outside - asserted;
      subB / intB  at least 8 (one model origin), and every one of them starts inside A's sphere of radius 1.5: B's hits outside A are
            never kept (Csg.fs:27-44), so no cull of the item can lose one - asserted."""
    ref = P.reference(prim, xf, structure)
    rays, at_origin, info = ref["rays"], P.origin_hits(ref), ref["info"]
    unbounded = prim == "plane" and structure.endswith("A")
    assert (info["items"], info["unbounded"]) == (4, int(unbounded))
    assert info["face_directions"] == (0 if unbounded else len({f.row for f in P.FACES[prim]}))
    assert not (at_origin & ~rays.expected).any()
    assert not at_origin[~np.isin(rays.band, P.PARALLEL_BANDS)].any()
    assert 0 < ref["blocked"].sum() < len(rays.o) and (ref["blocked"][at_origin] == 1).all()
    origin_of_target = P.matrix(P.flat_ops(xf))[1]
    if structure.endswith("B"):
        assert at_origin.sum() >= 8
        assert (np.linalg.norm(rays.o[at_origin] - origin_of_target, axis=1) < 1.5).all()
        return
    if structure == "intA":
        assert np.array_equal(at_origin, rays.expected)
        assert (np.linalg.norm(rays.o - origin_of_target, axis=1) < ref["reach"] / 1.1).all()
    assert at_origin.sum() >= 32
    if not _cullable(prim, xf):
        return
    if prim in P.CLOSED:
        centre, radius = ref["sphere"]
    elif structure == "subA":
        centre, radius = P.union_sphere([(prim, ref["m2w"][0]), ("sphere", ref["m2w"][1])])
    else:                                                           # an open A & the sphere that holds every origin: nothing lies outside the item
        centre, radius = P.union_sphere([(prim, ref["m2w"][0]), ("sphere", ref["m2w"][1])])
        assert (np.linalg.norm(rays.o - centre, axis=1) < radius).all()
        return
    far = P.line_distance(rays.o, rays.d, centre) > 2.0 * radius
    assert (far & at_origin).sum() >= 32, int((far & at_origin).sum())


def test_nine_directions_erase_the_op_cull_and_thirty_six_the_table():
    nine, three, many = (P.reference("cube", "rotate", s) for s in ("nine", "three", "many"))
    assert (nine["info"]["face_directions"], three["info"]["face_directions"], many["info"]["face_directions"]) == (9, 3, -1)
    assert nine["info"]["items"] == three["info"]["items"] == 4 and many["info"]["items"] == many["info"]["bounded_items"] == 15
    # the same union with one rotation for all three cubes has 3 directions and keeps its OP_CULL pair: two words more
    assert nine["info"]["program_words"] == three["info"]["program_words"] - 2
    assert np.array_equal(P.origin_hits(many), many["rays"].expected)
    for ref in (nine, many):
        at_origin = P.origin_hits(ref)
        assert not (at_origin & ~ref["rays"].expected).any()
        n = int((at_origin & ref["rays"].far).sum())
        assert n >= 32 and 3 * n >= int(at_origin.sum())


def _frame_facts(ref):
    view = ref["view"]
    den = ref["d"] @ ref["R"]
    hit, t, _, _, col = ref["closest"]
    at_origin = (hit != 0) & (t == 0.0) & (P.leaf_of_colour(col, hit) == 0)
    return view, den, at_origin


@pytest.mark.parametrize("prim,xf,kind", FRAME_CASES)
def test_frames_hold_a_parallel_row(prim, xf, kind):
    """From the oracle's ray_through_pixel: row py has |den| <= 1e-9 on every pixel (`band`: 1.3e-7 .. 1.7e-7); exactly the pixels with
    |den| < 1e-7 come back with t == 0 on the target and p == the ray's origin; the target's centre lies outside the cone of every
    wave (64 consecutive pixels, or an 8 x 8 block of a tile) that holds one, by more than two radii; the controls are seen; and the
    two kinds under a tile list are made of 8 x 8 blocks, the condition for k_classify to run."""
    ref = P.frame_reference(prim, xf, kind)
    view, den, at_origin = _frame_facts(ref)
    row = ref["ys"] == view.py
    assert row.sum() >= 30
    assert P.waves_of(view)[1] == (kind in ("tiles", "jitter"))
    if kind == "band":
        assert ((np.abs(den[row]) > 1.3e-7) & (np.abs(den[row]) < 1.7e-7)).all() and not at_origin[row].any()
    else:
        assert (np.abs(den[row]) <= 1e-9).all()
    parallel = np.abs(den) < P.K_EPS
    assert (np.abs(np.abs(den) - P.K_EPS) > 1e-10).all(), "a pixel too close to the rule to call"
    assert np.array_equal(at_origin, parallel)
    start = (ref["o"] + P.SLIGHT_OFFSET * ref["d"])[at_origin]
    assert (np.abs(ref["closest"][2][at_origin] - start) <= H.TIGHT * (1.0 + np.abs(start))).all()
    rows = sorted(set(ref["ys"][parallel].tolist()))
    if xf == "tall":
        assert len(rows) >= 5, "a band of rows under |row| = 1e-3"
    else:
        assert rows == ([] if kind == "band" else [view.py])
    if ref["sphere"] is not None and parallel.any():
        clear = P.wave_clearances(view, list(zip(ref["xs"][parallel].tolist(), ref["ys"][parallel].tolist())), ref["sphere"][0])
        assert min(clear.values()) > 2.0 * ref["sphere"][1]
        assert (P.line_distance(ref["o"][parallel], ref["d"][parallel], ref["sphere"][0]) > 2.0 * ref["sphere"][1]).all()
    leaf = P.leaf_of_colour(ref["closest"][4], ref["closest"][0])
    assert (leaf >= 10).sum() >= 20 and len(set(leaf[leaf >= 10].tolist())) >= 2
    if kind == "jitter":                                            # which pixels still hold a parallel sample: sample 0 as above, sample 1 ...
        _, d1, _, ys1 = P.pixel_rays(view, sample=1)
        par1 = np.abs(d1 @ ref["R"]) < P.K_EPS
        if xf == "tall":
            assert par1.any() and sorted(set(ys1[par1].tolist())) != rows
        else:
            assert not par1.any()
    info = P.host_facts(P.build_frame_scene, prim, xf, ref)[0]
    assert (info["items"], info["unbounded"]) == (4, int(prim == "plane"))


@pytest.mark.parametrize("kind", P.SHADOW_KINDS)
def test_shadow_rays_run_along_the_occluder_face(kind):
    """The shadow rays rebuilt from the oracle's primary hits: all of them (directional) or those of pixel row py (point) have
    |den| <= 1e-9 against the cube's y faces; of those, exactly the ones that start inside the column over the bottom face are blocked
    by it - none of the others in the column is; every ray's line passes the cube's sphere at more than two radii, and the sphere's
    centre lies outside the cone of every wave's shadow rays by as much."""
    ref = P.shadow_reference(kind)
    den = ref["sd"] @ ref["R"]
    parallel = np.abs(den) <= 1e-9
    assert not ((np.abs(den) > 1e-9) & (np.abs(den) < 1e-5)).any()
    view = ref["view"]
    if kind == "directional":
        assert parallel.all()
    else:
        assert parallel.sum() >= 5 and set(ref["ys"][parallel].tolist()) == {view.py} and parallel[ref["ys"] == view.py].all()
    model = ref["so"] @ ref["W"][:, :3].T + ref["W"][:, 3]
    in_column = (np.abs(model[:, 0]) < 0.5) & (np.abs(model[:, 2]) < 0.5) & (model[:, 1] > -0.5)
    assert (np.abs(np.abs(model[:, [0, 2]]) - 0.5) > 1e-9).all(), "a receiver point on the column's edge, where rounding decides"
    on_ball = ref["hit_leaf"] == 1
    by_cube = parallel & in_column
    assert by_cube.sum() >= 4 and (ref["blocked"][by_cube] == 1).all()
    lit_in_column = in_column & ~parallel & on_ball
    if kind == "point":
        assert lit_in_column.sum() >= 4, "the column is dark on one pixel row only"
    centre, radius = ref["sphere"]
    assert (P.line_distance(ref["so"], ref["sd"], centre) > 2.0 * radius).all()
    waves, _ = P.waves_of(view)
    wave = np.array([waves[p] for p in zip(ref["xs"].tolist(), ref["ys"].tolist())])
    for key in set(wave[by_cube].tolist()):
        sel = wave == key
        if kind == "point":                                         # the cone's apex is the light; it points at the receiver
            clear = P.cone_clearance(ref["light"], 0.0, -ref["sd"][sel], centre)
        else:
            spread = np.linalg.norm(ref["so"][sel] - ref["so"][sel][0], axis=1).max()
            clear = P.cone_clearance(ref["so"][sel][0], spread, ref["sd"][sel], centre)
        assert clear > 2.0 * radius, (key, clear, radius)
    assert 0.03 < (ref["frame"].sum(axis=2) > 0).mean()


@functools.lru_cache(maxsize=None)
def _mirror_facts():
    view, s, angle, centre = P.mirror_layout()
    orc = O.Oracle()
    P.build_mirror_scene(orc)
    o, d, xs, ys = P.pixel_rays(view)
    hit, t, p, n, col = orc.closest(o + P.SLIGHT_OFFSET * d, d)
    on_mirror = (hit != 0) & (np.abs(col - 0.9).max(axis=1) < 1e-12)
    rd = d - 2.0 * d[:, 1:2] * np.array([0.0, 1.0, 0.0])            # Shading.fs: reflect about the mirror's normal
    ro = p + P.SLIGHT_OFFSET * rd
    again = orc.closest(ro[on_mirror], rd[on_mirror])
    orc.close()
    out = (o, d, xs[on_mirror], ys[on_mirror], ro[on_mirror], rd[on_mirror])
    for a in out + tuple(again):
        a.setflags(write=False)
    return (view,) + out + (again,)


def test_reflected_rays_run_along_the_cube_face():
    info, m2w, w2m = P.host_facts(P.build_mirror_scene)
    assert (info["items"], info["unbounded"], info["face_directions"]) == (4, 1, 3)
    view, _, _, xs, ys, ro, rd, (hit, t, _, _, col) = _mirror_facts()
    den = rd @ w2m[1][1, :3]
    row = ys == view.py
    assert row.sum() >= 60 and (np.abs(den[row]) <= 1e-9).all() and (np.abs(den[~row]) > 1e-5).all()
    at_origin = (hit != 0) & (t == 0.0) & (P.leaf_of_colour(col, hit) == 1)
    assert at_origin.sum() >= 5 and set(ys[at_origin].tolist()) == {view.py}
    centre, radius = P.bounding_sphere("cube", m2w[1])
    assert (P.line_distance(ro[at_origin], rd[at_origin], centre) > 2.0 * radius).all()


# =============================================================================================================================
# GPU half

# A context of the module's own: the tests switch classify_pixels and coherent_waves.
@pytest.fixture(scope="module")
def ctx():
    c = ft.Context(device=0)
    yield c
    c.close()


def _check_explicit(ctx, ref, what):
    rays, want = ref["rays"], ref["closest"]
    got = ctx.closest(rays.o, rays.d)
    at_origin = P.origin_hits(ref)
    print(f"{what}: {len(rays.o)} rays, {int(want[0].sum())} hits, {int(at_origin.sum())} at the origin, {int((at_origin & rays.far).sum())} of them past the sphere")
    H.assert_hits_match(got, want, what=what)
    assert (got[1][at_origin] == 0.0).all() and (want[1][at_origin] == 0.0).all(), f"{what}: an origin hit with t != 0"
    assert np.array_equal(P.leaf_of_colour(got[4], got[0]), P.leaf_of_colour(want[4], want[0])), f"{what}: leaves differ"
    blocked = ctx.blocked(rays.o, rays.d, rays.max_dist)
    diff = np.nonzero(blocked != ref["blocked"])[0]
    assert diff.size == 0, f"{what}: blocked differs on {diff.size} rays, first {diff[:5]}"
    # the sparse route: at most 8 rays a call - the far origin hits first, then a stride through the rest
    pick = np.concatenate([np.nonzero(at_origin & rays.far)[0][:48], np.nonzero(at_origin & ~rays.far)[0][:16], np.arange(0, len(rays.o), max(1, len(rays.o) // 32))])
    for k in range(0, len(pick), 8):
        sel = pick[k:k + 8]
        part = ctx.closest(rays.o[sel], rays.d[sel])
        H.assert_hits_match(part, tuple(a[sel] for a in want), what=f"{what}, rays {sel.tolist()} alone")
        assert (part[1][at_origin[sel]] == 0.0).all()
        assert np.array_equal(ctx.blocked(rays.o[sel], rays.d[sel], rays.max_dist[sel]), ref["blocked"][sel]), f"{what}, rays {sel.tolist()} alone: blocked differs"


@gpu
@pytest.mark.parametrize("alone", [False, True], ids=["among-controls", "alone"])
@pytest.mark.parametrize("prim,xf", BARE_CASES)
def test_explicit_rays(ctx, prim, xf, alone):
    ref = P.reference(prim, xf, "bare", alone)
    P.build_scene(ctx, prim, xf, "bare", ref["controls"])
    _check_explicit(ctx, ref, f"{prim} {xf}{' alone' if alone else ''}")


@gpu
@pytest.mark.parametrize("prim,xf,structure", CSG_CASES)
def test_explicit_rays_under_csg(ctx, prim, xf, structure):
    ref = P.reference(prim, xf, structure)
    P.build_scene(ctx, prim, xf, structure, ref["controls"], reach=ref["reach"])
    _check_explicit(ctx, ref, f"{prim} {xf} {structure}")


@gpu
@pytest.mark.parametrize("structure,xf", [("nine", "rotate"), ("nine", "tall"), ("many", "rotate"), ("many", "shear")])
def test_explicit_rays_past_the_direction_limits(ctx, structure, xf):
    ref = P.reference("cube", xf, structure)
    P.build_scene(ctx, "cube", xf, structure, ref["controls"])
    assert ctx.scene_info()["face_directions"] == (9 if structure == "nine" else -1)
    _check_explicit(ctx, ref, f"{structure} {xf}")


def _render_variants(ctx, render):
    """render() under classify_pixels x coherent_waves; the four results, defaults first."""
    out = []
    try:
        for classify, coherent in ((1, 1), (0, 1), (1, 0), (0, 0)):
            ctx.set_option("classify_pixels", classify)
            ctx.set_option("coherent_waves", coherent)
            out.append(render())
    finally:
        ctx.set_option("classify_pixels", 1)
        ctx.set_option("coherent_waves", 1)
    return out


def _check_frame(got, st, want, ost, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pixels differ"
    nan = np.isnan(want)
    worst = H.assert_frames_match(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what=what)
    print(f"{what}: worst pixel {worst:.3e}")
    assert worst < 1e-6, f"{what}: worst pixel {worst:.3e}"
    assert st["rays_reference_equivalent"] == ost["rays_traced"]


@gpu
@pytest.mark.parametrize("prim,xf,kind", FRAME_CASES)
def test_frames_with_a_parallel_row(ctx, prim, xf, kind):
    ref = P.frame_reference(prim, xf, kind)
    view, xs, ys, want = ref["view"], ref["xs"], ref["ys"], ref["closest"]
    what = f"{prim} {xf} {kind}"
    P.build_frame_scene(ctx, prim, xf, ref)
    cam = P.camera(view)
    planes = _render_variants(ctx, lambda: ctx.render_aov(cam, view.w, view.h, view.spp, view.jitter, tiles=view.tiles, channels=PLANES))
    whit = want[0]
    at_origin = (whit != 0) & (want[1] == 0.0)
    want_leaf = P.leaf_of_colour(want[4], whit)
    want_leaf = np.where(want_leaf >= 10, want_leaf - 10 + P.frame_target(prim)[2], want_leaf)   # the controls are the leaves after the target's
    for got, route in zip(planes, ("defaults", "unclassified", "per-lane", "unclassified per-lane")):
        ghit = (got["leaf"][ys, xs] >= 0).astype(np.int32)
        print(f"{what} {route}: {int(ghit.sum())} hits of {len(xs)} rays, oracle {int(whit.sum())}, {int(at_origin.sum())} at the origin")
        H.assert_hits_match((ghit, got["t"][ys, xs], got["p"][ys, xs], got["n"][ys, xs], got["colour"][ys, xs]), want, what=f"{what} {route}")
        assert (got["t"][ys, xs][at_origin] == 0.0).all(), f"{what} {route}: an origin hit with t != 0"
        assert np.array_equal(got["leaf"][ys, xs], want_leaf), f"{what} {route}: leaves differ"
        for k in PLANES:
            assert np.array_equal(got[k], planes[0][k], equal_nan=k in ("t", "p", "n", "colour")), f"{what}: plane {k} of {route} differs from the defaults'"
    before = ctx.classify_reuse()
    frames = _render_variants(ctx, lambda: ctx.render(cam, view.w, view.h, view.spp, view.jitter, tiles=view.tiles))
    after = ctx.classify_reuse()
    classified = kind in ("tiles", "jitter") and prim != "plane"    # (no classification beside an unbounded item)
    assert (after["classified"] + after["reused"] > before["classified"] + before["reused"]) == classified, (before, after)
    for (frame, _), route in zip(frames[1:], ("unclassified", "per-lane", "unclassified per-lane")):
        assert np.array_equal(frame, frames[0][0], equal_nan=True), f"{what}: the {route} frame differs from the defaults' on {int(np.any(frame != frames[0][0], axis=2).sum())} pixels"
    _check_frame(frames[0][0], frames[0][1], ref["frame"], ref["stats"], what)


@gpu
@pytest.mark.parametrize("kind", P.SHADOW_KINDS)
def test_shadow_rays_along_the_occluder_face(ctx, kind):
    ref = P.shadow_reference(kind)
    view = ref["view"]
    P.build_shadow_scene(ctx, kind, ref["light"])
    assert ctx.scene_info()["items"] == 3 and ctx.scene_info()["face_directions"] == 3
    got = ctx.blocked(ref["so"], ref["sd"], ref["dist"])
    diff = np.nonzero(got != ref["blocked"])[0]
    assert diff.size == 0, f"{kind}: blocked differs on {diff.size} shadow rays, first {diff[:5]}"
    frames = _render_variants(ctx, lambda: ctx.render(P.camera(view), view.w, view.h, 1, np.zeros((1, 2))))
    for (frame, _), route in zip(frames[1:], ("unclassified", "per-lane", "unclassified per-lane")):
        assert np.array_equal(frame, frames[0][0], equal_nan=True), f"{kind}: the {route} frame differs from the defaults' on {int(np.any(frame != frames[0][0], axis=2).sum())} pixels"
    _check_frame(frames[0][0], frames[0][1], ref["frame"], ref["stats"], f"{kind} light")


@gpu
@pytest.mark.parametrize("max_depth", [2, 8])
def test_reflected_rays_along_the_cube_face(ctx, max_depth):
    view, o, d, *_ = _mirror_facts()
    orc = O.Oracle()
    P.build_mirror_scene(orc)
    want, ost = orc.render(P.camera(view), view.w, view.h, 1, np.zeros((1, 2)), max_depth=max_depth, seed=ft.DEFAULT_SEED)
    want_rays = orc.colour_for_ray(o + P.SLIGHT_OFFSET * d, d, max_depth=max_depth)
    orc.close()
    P.build_mirror_scene(ctx)
    frames = _render_variants(ctx, lambda: ctx.render(P.camera(view), view.w, view.h, 1, np.zeros((1, 2)), max_depth=max_depth))
    for (frame, _), route in zip(frames[1:], ("unclassified", "per-lane", "unclassified per-lane")):
        assert np.array_equal(frame, frames[0][0], equal_nan=True), f"depth {max_depth}: the {route} frame differs from the defaults'"
    _check_frame(frames[0][0], frames[0][1], want, ost, f"mirror, depth {max_depth}")
    got_rays = ctx.colour_for_ray(o + P.SLIGHT_OFFSET * d, d, max_depth=max_depth)
    assert np.array_equal(np.isnan(got_rays), np.isnan(want_rays))
    err = H.pixel_errors(np.nan_to_num(got_rays), np.nan_to_num(want_rays))
    assert err.max() < 1e-6, f"colour_for_ray, depth {max_depth}: worst ray {err.max():.3e}"

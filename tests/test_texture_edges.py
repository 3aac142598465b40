"""Texture lookups exactly on cell, texel, seam and pole borders.

`surface_at` gives a hit its (u, v) and `textured_colour` turns it into a colour through comparisons between doubles; rays drawn
from continuous distributions never land on the borders those comparisons decide.  Here they do:

exact families  rays along a model axis from dyadic origins, so that (u, v) is exact (proved per case with Fractions in
                tests/texture_tools.py): every pair of the border values on plane, square, circle, the six cube faces and both
                solidCylinder caps under a grid, bare and under a power-of-two scale with a dyadic translation; a uv scale of 0
                (NaN); every texel border of seven image sizes with the wrap at ru == 1.0 and the clamp; the sphere's axis points,
                seam and poles; the primitives whose (u, v) is (0, 0); several images in one scene;
ladders         the sphere at generic points, the plane under a rotate uv function and a rotated cube, stepped across a border at
                +-2^-k, k = 10 .. 52, against mpmath at 60 digits; a rung closer than 2^-46 max(1, |coordinate|) is undecided;
function order  every sequence of 1 .. 4 of material / grid / image / hueShift / ignoreLight around a square, against the oracle.

The expectation is the independent reference of texture_tools; the oracle must equal it on the CPU wherever a case is kept.  The
device goes through `closest`, `colour_for_ray` at depth 0 (unlit surfaces) and at depth 1 (a black mirror over the textured plane),
`render_aov` and small frames under every kernel-selecting option.

Findings: see DESIGN.md §15.3."""
import functools
import itertools

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from . import texture_tools as X
from .test_aov import _pixel_rays

COLOUR_TOL = 1e-12                                                 # the suite's bound on a material colour (helpers.assert_hits_match)
CHUNK = 48                                                         # layers per scene
FACE_CASES = [(f, xf) for f in X.FACES for xf in (False, True)]
LADDER_NAMES = ["sphere u=0.5", "sphere seam", "sphere equator", "sphere texel column", "sphere texel row", "plane rotate 30", "plane rotate 90", "cube rotated"]
RESIDUE_FACES = {"cube_left", "cube_right", "cube_front", "cube_back", "cap_bottom"}   # tie_tools.RESIDUE_FACES: rotated in the reference


def assert_colours(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.nonzero(np.any(~(np.abs(got - want) <= COLOUR_TOL), axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} colours differ, first at {bad[:6]}: {got[bad[:3]]} vs {want[bad[:3]]}"


def closest_colours(b, o, d, what):
    hit, _, _, _, col = b.closest(o, d)
    assert hit.all(), f"{what}: rays {np.nonzero(hit == 0)[0][:8]} miss"
    return col


def agreement(got, want):
    return np.all(np.abs(np.asarray(got) - np.asarray(want)) <= COLOUR_TOL, axis=1)


def routes(b, o, d, what):
    """The colour of every ray through closest and through getColourForRay at depth 0 (every textured surface here ignores light)."""
    return {"closest": closest_colours(b, o, d, what), "colour_for_ray depth 0": b.colour_for_ray(o, d, max_depth=0)}


# =============================================================================================================================
# References, computed once per process and shared by the CPU and the GPU halves

@functools.lru_cache(maxsize=None)
def face_reference(face, xf):
    layers, cases = X.face_cases(face, xf)
    o, d = X.layer_rays(face, cases, xf)
    return layers, cases, o, d, X.expected_colours(cases, X.GRID)


@functools.lru_cache(maxsize=None)
def zero_reference(face):
    cases = X.zero_scale_cases(face)
    o, d = X.layer_rays(face, cases)
    return cases, o, d


@functools.lru_cache(maxsize=None)
def image_reference(w, h):
    img = X.image(w, h)
    cases = X.image_cases(w, h)
    o, d = X.layer_rays("plane", cases)
    return img, cases, o, d, X.expected_colours(cases, img)


def chunks(layers, cases):
    """(first layer, indices of the cases on layers first .. first + CHUNK - 1)."""
    for first in range(0, len(layers), CHUNK):
        idx = np.array([i for i, c in enumerate(cases) if first <= c.layer < first + CHUNK], dtype=np.int64)
        if idx.size:
            yield first, idx


def face_colours(b, face, xf, texture, layers, cases, o, d, what):
    """Both routes for every case, scene by scene."""
    out = {}
    for first, idx in chunks(layers, cases):
        X.build_layers(b, face, layers, texture, xf, chunk=(first, CHUNK))
        for route, col in routes(b, o[idx], d[idx], what).items():
            out.setdefault(route, np.zeros((len(cases), 3)))[idx] = col
    return out


@functools.lru_cache(maxsize=None)
def kept_on_oracle(face, xf):
    """The cases on which the oracle equals the residue-free reference (every case, outside the faces the reference text rotates)."""
    layers, cases, o, d, want = face_reference(face, xf)
    got = face_colours(O.Oracle(), face, xf, X.GRID, layers, cases, o, d, f"oracle {face}")
    for route, col in got.items():
        assert np.array_equal(agreement(col, want), agreement(got["closest"], want)), route
    return agreement(got["closest"], want)


@functools.lru_cache(maxsize=None)
def ladders():
    """name -> (scene builder, rungs, allowed colours per rung)."""
    img = X.image(5, 7)
    sphere = lambda tex: (lambda b: X.build_single(b, X.prim_node("sphere"), tex))
    out = {}
    for name, which, border, other, tex in (("sphere u=0.5", 0, 0.5, 0.3, X.GRID), ("sphere seam", 0, 1.0, 0.3, X.GRID), ("sphere equator", 1, 0.5, 0.3, X.GRID),
                                            ("sphere texel column", 0, 2.0 / 5.0, 0.3, img), ("sphere texel row", 1, 3.0 / 7.0, 0.3, img)):
        rungs = X.sphere_ladder(which, border, other)
        out[name] = (sphere(tex), rungs, X.ladder_expectation(rungs, tex.colour, border, which))
    for deg in (30.0, 90.0):
        ops = ((1.0, H.deg(deg), 0.0),)
        rungs = X.rotated_plane_ladder(H.deg(deg))
        out[f"plane rotate {deg:g}"] = ((lambda b, ops=ops: X.build_single(b, X.prim_node("plane"), X.GRID, ops)), rungs, X.ladder_expectation(rungs, X.GRID.colour, 0.5))
    rungs = X.rotated_cube_ladder()
    out["cube rotated"] = ((lambda b: X.build_single(b, X.prim_node("cube", (("rotate", X.CUBE_AXIS, X.CUBE_ANGLE),)), X.GRID)), rungs,
                           X.ladder_expectation(rungs, X.GRID.colour, 0.5))
    return out


def ladder_verdicts(b, name):
    """Per rung: whether the builder's colour is one of the allowed ones, on both routes."""
    build, rungs, allowed = ladders()[name]
    build(b)
    o, d = np.array([r.o for r in rungs]), np.array([r.d for r in rungs])
    ok = np.ones(len(rungs), dtype=bool)
    for col in routes(b, o, d, name).values():
        ok &= np.array([any(np.all(np.abs(c - np.array(a)) <= COLOUR_TOL) for a in al) for c, al in zip(col, allowed)])
    return ok


# =============================================================================================================================
# CPU half

def test_reference_on_hand_worked_values():
    g, E = X.grid_first, X.E53
    # the four-way rule (Texture.fs:26-29) with each operand on, just below and just above 0.5
    below, above = 0.5 - X.E54, 0.5 + E
    assert g(below, below) and not g(below, 0.5) and not g(below, above)           # u < 0.5: colour1 only with v < 0.5
    assert not g(0.5, below) and not g(0.5, 0.5) and not g(0.5, above)            # u == 0.5: neither strict test holds
    assert not g(above, below) and not g(above, 0.5) and g(above, above)          # u > 0.5: colour1 only with v > 0.5
    assert X.repeat_one(-X.E60) == 1.0 and X.repeat_one(-0.25) == 0.75 and X.repeat_one(3.5) == 0.5 and X.repeat_one(2.0 ** 51 + 0.5) == 0.5
    assert X.repeat_one(1e300) == 0.0 and X.repeat_one(-0.0) == 0.0 and X.repeat_one(1.0 - E) == 1.0 - E
    assert float(2 ** 52) == 2.0 ** 52 + 0.5                                       # 2^52 + 0.5 is no double: TARGETS holds 2^52 and 2^51 + 0.5
    nan = X.repeat_one(X.fdiv(0.5, 0.0))
    assert nan != nan and not g(nan, 0.25) and not g(0.25, nan) and not g(0.75, nan)
    # Image.fs:29-31 on a 5 x 7 image: x == width wraps into the next row, the last row and rv == 1.0 take the clamp, NaN texel 0
    t = lambda u, v: X.image_texel(5, 7, u, v)
    assert t(0.0, 0.0) == 0 and t(0.2, 0.0) == 1 and t(np.nextafter(0.2, 0), 0.0) == 0 and t(0.0, 1.0 / 7.0) == 5
    assert t(-X.E60, 0.0) == 5 and t(-X.E60, 0.5) == 3 * 5 + 5 and t(-X.E60, 6.5 / 7.0) == 34 and t(0.3, -X.E60) == 34 and t(nan, 0.5) == 0 and t(0.5, nan) == 0
    assert X.image_texel(1, 1, -X.E60, -X.E60) == 0 and X.image_texel(1, 9, -X.E60, 0.0) == 1 and X.image_texel(9, 1, -X.E60, 0.0) == 8
    assert X.hue((1, 2, 3)) == (3, 1, 2) and X.hue((1, 2, 3), 2) == (2, 3, 1) and X.hue((1, 2, 3), 3) == (1, 2, 3)
    # the sphere's axis points: fl(pi/2) / (2 fl(pi)) is exactly 0.25
    for e, uv in X.AXIS_UV.items():
        assert X.sphere_uv([float(c) for c in e]) == uv, e
    assert X.sphere_uv([-1.0, 0.0, -0.0]) == (0.0, 0.5)


@pytest.mark.parametrize("face,xf", FACE_CASES)
def test_exact_faces_reference_vs_oracle(face, xf, capsys):
    layers, cases, o, d, want = face_reference(face, xf)
    assert len(cases) == len(X.TARGETS) ** 2
    for c in cases:
        assert X.prove_face_case(face, c.a, c.b, X.LAYER_STEP * c.layer, xf), (face, c)
        assert all(X.same_bits(g, w) for g, w in zip(X.apply_ops(c.ops, c.a, c.b), c.target)), (face, c)
    firsts = {(X.repeat_one(c.target[0]), X.repeat_one(c.target[1])) for c in cases}
    for ru in (0.5 - X.E54, 0.5, 0.5 + X.E53):                      # every branch with each operand on, just below and just above 0.5
        for rv in (0.5 - X.E54, 0.5, 0.5 + X.E53):
            assert (ru, rv) in firsts
    assert {tuple(w) for w in want} == {X.GRID.c1, X.GRID.c2}
    kept = kept_on_oracle(face, xf)
    with capsys.disabled():
        print(f"\n  {face}{' under XF' if xf else ''}: {len(layers)} layers, {len(cases)} cases, oracle agrees on {int(kept.sum())}", end="")
    if face in RESIDUE_FACES:
        assert kept.mean() >= 0.5, f"{face}: the oracle agrees on {kept.mean():.0%} only"
        off = [cases[i] for i in np.nonzero(~kept)[0]]              # the residue decides only on a face's own border
        assert all(c.a in (0.0, 1.0) or c.b in (0.0, 1.0) for c in off), f"{face}: the oracle differs inside the face: {off[:4]}"
    else:
        assert kept.all(), f"{face}: the oracle differs from the reference on cases {[cases[i] for i in np.nonzero(~kept)[0][:4]]}"


@pytest.mark.parametrize("face", list(X.FACES))
def test_zero_uv_scale_reference_vs_oracle(face):
    """u / 0 is inf or NaN and NaN after repeat: the grid gives colour2, the image texel 0 - if the builders take a zero scale at all."""
    cases, o, d = zero_reference(face)
    img = X.image(5, 7)
    for tex, want in ((X.GRID, X.GRID.c2), (img, img.texel(0))):
        assert all(tex.colour(*X.apply_ops(c.ops, c.a, c.b)) == want for c in cases)
        orc = O.Oracle()
        X.build_layers(orc, face, X.ZERO_OPS, tex)
        for route, col in routes(orc, o, d, face).items():
            assert_colours(col, np.tile(want, (len(cases), 1)), f"oracle, zero uv scale, {face}, {route}")


@pytest.mark.parametrize("w,h", X.IMAGE_SIZES)
def test_image_borders_reference_vs_oracle(w, h):
    img, cases, o, d, want = image_reference(w, h)
    texels = [X.image_texel(w, h, c.a, c.b) for c in cases]
    assert set(texels) == set(range(w * h))
    wrapped = [c for c in cases if X.repeat_one(c.a) == 1.0]
    assert len({X.image_texel(w, h, c.a, c.b) for c in wrapped}) >= min(h, w * h - 1) and any(X.repeat_one(c.b) == 1.0 for c in cases)
    orc = O.Oracle()
    X.build_layers(orc, "plane", [()], img)
    for route, col in routes(orc, o, d, "image").items():
        assert_colours(col, want, f"oracle, image {w}x{h}, {route}")


SPHERE_TEXTURES = {"grid": X.GRID, "8x4": X.image(8, 4), "5x7": X.image(5, 7)}


def sphere_axis_expected(xf, tex):
    o, d, normals = X.sphere_axis_rays(xf)
    uv = [X.sphere_uv(n) for n in normals]
    return o, d, uv, np.array([tex.colour(u, v) for u, v in uv])


@pytest.mark.parametrize("xf", list(X.SPHERE_XF))
def test_sphere_axis_points_reference_vs_oracle(xf):
    for name, tex in SPHERE_TEXTURES.items():
        o, d, uv, want = sphere_axis_expected(xf, tex)
        assert uv[:6] == [X.AXIS_UV[e] for e in X.AXES] and (xf != "unit" or uv[6:] == [(1.0, 0.5), (0.0, 0.5)])
        if name != "grid":                                          # the seam gives column 0, both poles row 0
            assert X.image_texel(tex.w, tex.h, *uv[1]) % tex.w == 0 and X.image_texel(tex.w, tex.h, *uv[2]) < tex.w and X.image_texel(tex.w, tex.h, *uv[3]) < tex.w
        orc = O.Oracle()
        X.build_single(orc, X.prim_node("sphere", X.SPHERE_XF[xf]), tex)
        for route, col in routes(orc, o, d, "sphere axis").items():
            assert_colours(col, want, f"oracle, sphere axis points, {xf}, {name}, {route}")


FLAT_CASES = [(n, k, s) for n in X.flat_uv_nodes() for k in range(len(X.FLAT_OPS)) for s in (0, 1, 2)]


def check_flat_uv(b, name, k, shifts, what):
    node, (o, d) = X.flat_uv_nodes()[name]
    img = X.image(5, 7)
    for tex, base in ((X.GRID, X.GRID.c1), (img, img.texel(0))):
        X.build_single(b, node, tex, X.FLAT_OPS[k], hue_shifts=shifts)
        hit, _, _, _, col = b.closest(o, d)
        m = hit.astype(bool)
        assert m.sum() >= 32, f"{what} {name}: {int(m.sum())} hits"
        want = np.tile(X.hue(base, shifts), (int(m.sum()), 1))
        assert_colours(col[m], want, f"{what} {name}, uv functions {k}, {shifts} hueShifts, closest")
        assert_colours(b.colour_for_ray(o, d, max_depth=0)[m], want, f"{what} {name}, uv functions {k}, {shifts} hueShifts, colour_for_ray")


@pytest.mark.parametrize("name,k,shifts", FLAT_CASES)
def test_flat_uv_primitives_on_oracle(name, k, shifts):
    check_flat_uv(O.Oracle(), name, k, shifts, "oracle")


def check_image_stack(b, what):
    textures = X.build_image_stack(b)
    cases = X.image_stack_cases(textures)
    o, d = X.layer_rays("square", cases)
    want = np.array([textures[-c.layer].colour(c.a, c.b) for c in cases])
    for route, col in routes(b, o, d, what).items():
        assert_colours(col, want, f"{what}: images in one scene, {route}")
    return want


def test_images_in_one_scene_on_oracle():
    want = check_image_stack(O.Oracle(), "oracle")
    assert len({tuple(w) for w in want}) >= 1 + 21 + 35 + 9 + 9        # the texels of the five images: every square returns its own


@pytest.mark.parametrize("name", LADDER_NAMES)
def test_ladder_caps_and_oracle(name, capsys):
    _, rungs, allowed = ladders()[name]
    share = X.undecided_share(rungs)
    ok = ladder_verdicts(O.Oracle(), name)
    decided = np.array([r.decided for r in rungs])
    with capsys.disabled():
        print(f"\n  {name}: {int((~decided).sum())} of {len(rungs)} rungs undecided; the oracle takes the reference's colour on {int(ok[decided].sum())} of {int(decided.sum())} others", end="")
    assert len(rungs) == 86 and share <= X.MAX_UNDECIDED, f"{name}: {share:.0%} undecided"
    assert all(len(a) == 1 for a, r in zip(allowed, rungs) if r.decided) and all(len(a) == 2 for a, r in zip(allowed, rungs) if not r.decided)
    sides = {(r.side, tuple(next(iter(a)))) for a, r in zip(allowed, rungs) if r.decided}
    assert len(sides) == 2, f"{name}: the two sides of the border must have one colour each, and differ: {sides}"
    assert ok.all(), f"{name}: the oracle leaves the allowed colours on rungs {np.nonzero(~ok)[0][:8]}"


def order_results(b, seqs):
    o, d = X.build_order_scene(b, seqs)
    hit, _, _, _, col = b.closest(o, d)
    assert hit.all()
    return col, b.colour_for_ray(o, d, max_depth=0)


@functools.lru_cache(maxsize=None)
def order_oracle():
    return [order_results(O.Oracle(), list(seqs)) for seqs in X.order_scenes()]


def test_function_order_is_alive_on_the_oracle():
    assert len(X.SEQUENCES) == 780
    col = np.concatenate([c for c, _ in order_oracle()])
    shaded = np.concatenate([s for _, s in order_oracle()])
    outcome = {}
    for k, seq in enumerate(X.SEQUENCES):
        want, lit = X.order_expected(seq)
        assert np.all(np.abs(col[k] - np.array(want)) <= COLOUR_TOL), f"{seq}: the oracle's colour {col[k]}, by the text {want}"
        assert lit != bool(np.all(np.abs(shaded[k] - np.array(want)) <= COLOUR_TOL)), f"{seq}: applyLighting should be {lit}"
        outcome[seq] = (tuple(col[k]), tuple(shaded[k]))
    for n in (2, 3, 4):
        assert len({v for s, v in outcome.items() if len(s) == n}) >= 4
    three = [s for s in X.SEQUENCES if len(s) == 3]
    swapped = sum(outcome[s][0] != outcome[(s[0], s[2], s[1])][0] for s in three)
    assert swapped >= len(three) / 5, f"swapping the last two functions changes {swapped} of {len(three)}"


def mirror_scene(b, tex, ops=()):
    """The textured, unlit plane at y = 0 under a black mirror at y = 2 (colour 0, reflectance 1, shineyness 0: its own terms are 0, so
    the ray's colour is the reflected one)."""
    mirror = lambda bb: [bb.material(bb.translate((0.0, 2.0, 0.0), bb.primitive(ft.PLANE)), colour=(0, 0, 0), reflectance=1.0, shineyness=0.0)]
    X.build_single(b, X.prim_node("plane"), tex, ops, extra=mirror)


@functools.lru_cache(maxsize=None)
def mirror_reference(which):
    """Rays straight up from y = 1: the reflected ray comes down along the same x and z."""
    if which == "grid":
        _, cases, o, d, want = face_reference("plane", False)
        keep = [i for i, c in enumerate(cases) if c.layer == 0]
        tex, cases, want = X.GRID, [cases[i] for i in keep], want[keep]
    else:
        tex, cases, _, _, want = image_reference(*which)
    o = np.array([[c.a, 1.0, c.b] for c in cases])
    return tex, o, np.tile([0.0, 1.0, 0.0], (len(cases), 1)), want


MIRROR_CASES = ["grid", (5, 7), (8, 4)]
MIRROR_IDS = ["grid", "5x7", "8x4"]


@pytest.mark.parametrize("which", MIRROR_CASES, ids=MIRROR_IDS)
def test_mirror_route_on_oracle(which):
    tex, o, d, want = mirror_reference(which)
    assert len(want) >= 100
    orc = O.Oracle()
    mirror_scene(orc, tex)
    assert_colours(orc.colour_for_ray(o, d, max_depth=1), want, f"oracle, mirror over {which}")
    assert np.all(orc.colour_for_ray(o, d, max_depth=0) == 0.0)


MIRROR_LADDERS = ["plane rotate 30", "plane rotate 90"]


def mirror_ladder_verdicts(b, name):
    """The rotated plane's ladders through the mirror: rays straight up from under it, at the rungs' x and z."""
    _, rungs, allowed = ladders()[name]
    mirror_scene(b, X.GRID, ((1.0, H.deg(float(name.split()[-1])), 0.0),))
    o = np.array([[r.o[0], 1.0, r.o[2]] for r in rungs])
    col = b.colour_for_ray(o, np.tile([0.0, 1.0, 0.0], (len(rungs), 1)), max_depth=1)
    return np.array([any(np.all(np.abs(c - np.array(a)) <= COLOUR_TOL) for a in al) for c, al in zip(col, allowed)])


@pytest.mark.parametrize("name", MIRROR_LADDERS)
def test_mirror_ladders_on_oracle(name):
    assert mirror_ladder_verdicts(O.Oracle(), name).all()


# =============================================================================================================================
# GPU half

@pytest.mark.gpu
@pytest.mark.parametrize("face,xf", FACE_CASES)
def test_exact_faces_on_device(hip, face, xf):
    """Every case against the residue-free reference; the oracle agrees on the kept ones (asserted by the CPU half)."""
    layers, cases, o, d, want = face_reference(face, xf)
    for route, col in face_colours(hip, face, xf, X.GRID, layers, cases, o, d, face).items():
        assert_colours(col, want, f"{face}{' under XF' if xf else ''}, {route}")


@pytest.mark.gpu
@pytest.mark.parametrize("face", list(X.FACES))
def test_zero_uv_scale_on_device(hip, face):
    cases, o, d = zero_reference(face)
    img = X.image(5, 7)
    for tex, want in ((X.GRID, X.GRID.c2), (img, img.texel(0))):
        X.build_layers(hip, face, X.ZERO_OPS, tex)
        for route, col in routes(hip, o, d, face).items():
            assert_colours(col, np.tile(want, (len(cases), 1)), f"zero uv scale, {face}, {route}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", X.IMAGE_SIZES)
def test_image_borders_on_device(hip, w, h):
    img, cases, o, d, want = image_reference(w, h)
    X.build_layers(hip, "plane", [()], img)
    for route, col in routes(hip, o, d, "image").items():
        assert_colours(col, want, f"image {w}x{h}, {route}")


@pytest.mark.gpu
@pytest.mark.parametrize("xf", list(X.SPHERE_XF))
def test_sphere_axis_points_on_device(hip, xf):
    """The closed form: u in {0.5, 1.0, 0.75, 0.25}, v in {0.5, 0, 1}: atan2 and asin must round these arguments correctly."""
    for name, tex in SPHERE_TEXTURES.items():
        o, d, _, want = sphere_axis_expected(xf, tex)
        X.build_single(hip, X.prim_node("sphere", X.SPHERE_XF[xf]), tex)
        for route, col in routes(hip, o, d, "sphere axis").items():
            assert_colours(col, want, f"sphere axis points, {xf}, {name}, {route}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(X.flat_uv_nodes()))
def test_flat_uv_primitives_on_device(hip, name):
    for n, k, shifts in FLAT_CASES:
        if n == name:
            check_flat_uv(hip, name, k, shifts, "device")


@pytest.mark.gpu
def test_images_in_one_scene_on_device(hip):
    check_image_stack(hip, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("name", LADDER_NAMES)
def test_ladders_on_device(hip, name):
    ok = ladder_verdicts(hip, name)
    rungs = ladders()[name][1]
    assert ok.all(), f"{name}: rungs {np.nonzero(~ok)[0][:8]} (decided: {[rungs[i].decided for i in np.nonzero(~ok)[0][:8]]}) leave the allowed colours"


@pytest.mark.gpu
def test_function_order_on_device(hip):
    """closest's colour and colour_for_ray at depth 0 (which shows whether applyLighting survived) for all 780 sequences."""
    for k, (seqs, (want_col, want_shaded)) in enumerate(zip(X.order_scenes(), order_oracle())):
        col, shaded = order_results(hip, list(seqs))
        assert_colours(col, want_col, f"function order, scene {k}, closest")
        assert_colours(col, np.array([X.order_expected(s)[0] for s in seqs]), f"function order, scene {k}, closest against the text")
        assert np.allclose(shaded, want_shaded, rtol=1e-9, atol=COLOUR_TOL), f"function order, scene {k}: colour_for_ray differs for {[seqs[i] for i in np.nonzero(~np.all(np.isclose(shaded, want_shaded, rtol=1e-9, atol=COLOUR_TOL), axis=1))[0][:4]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("which", MIRROR_CASES, ids=MIRROR_IDS)
def test_mirror_route_on_device(hip, which):
    """k_bounce's lookup: colour_for_ray at depth 1 off a black mirror, the reflected ray keeping its exact x and z."""
    tex, o, d, want = mirror_reference(which)
    mirror_scene(hip, tex)
    assert_colours(hip.colour_for_ray(o, d, max_depth=1), want, f"mirror over {which}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", MIRROR_LADDERS)
def test_mirror_ladders_on_device(hip, name):
    ok = mirror_ladder_verdicts(hip, name)
    assert ok.all(), f"{name} through the mirror: rungs {np.nonzero(~ok)[0][:8]} leave the allowed colours"


def frame_scene(b, lights, mesh=True, only_mesh=False, lit=True):
    """A textured plane, sphere, cube and solidCylinder and a textured bspMesh 0 (an octahedron)."""
    img = X.image(5, 7)
    tris = np.array(X.OCTA, dtype=np.float64).reshape(-1, 9)
    b.clear()
    objs = []
    if not only_mesh:
        objs.append(b.texture_grid(X.GRID.c1, X.GRID.c2, [(0.0, 0.5, 0.5), (1.0, H.deg(30.0), 0.0)], b.translate((0, -1, 0), b.primitive(ft.PLANE))))
        objs.append(b.hue_shift(0.0, img.wrap(b, (), b.translate((-1.5, 0, 0), b.primitive(ft.SPHERE)))))
        objs.append(b.texture_grid(X.GRID.c2, X.GRID.c1, [(0.0, 0.25, 0.25)], b.transform([("rotate", X.CUBE_AXIS, X.CUBE_ANGLE), ("translate", (1.2, 0.0, 0.5))], b.primitive(ft.CUBE))))
        objs.append(img.wrap(b, [(0.0, 0.5, 0.5)], b.transform([("rotate", (1.0, 0.0, 0.0), H.deg(40.0)), ("translate", (0.0, -0.6, -1.6))], b.primitive(ft.SOLID_CYLINDER))))
    if mesh or only_mesh:
        node = b.transform([("scale", 0.6), ("translate", (0.0, 0.9, 0.3))], b.bsp_mesh(0, tris))
        objs.append(b.hue_shift(0.0, b.hue_shift(0.0, X.GRID.wrap(b, (), node))))
    b.set_objects(b.group(objs))
    b.add_directional((0.3, -1.0, 0.6), (1.0, 0.9, 0.8))
    if lights == "soft":
        b.add_soft_directional((-0.4, -1.0, 0.2), 3, H.deg(4.0), (0.5, 0.5, 0.6))
    b.commit()


FRAME_CASES = [("directional", True, False), ("soft", True, False), ("directional", False, False), ("directional", True, True)]
W, Hh, SPP = 64, 48, 2


@pytest.mark.gpu
@pytest.mark.parametrize("lights,mesh,only_mesh", FRAME_CASES)
def test_textured_frames_under_every_option(hip, lights, mesh, only_mesh):
    orc = O.Oracle()
    for b in (orc, hip):
        frame_scene(b, lights, mesh, only_mesh)
    cam = ft.make_camera((0.5, 2.0, -5.5), (0.0, 0.0, 0.0), (0, 1, 0), H.deg(50.0), W / Hh)
    jit = ft.jitter_pattern(SPP)
    want, _ = orc.render(cam, W, Hh, SPP, jit, seed=ft.DEFAULT_SEED)
    assert len({tuple(p) for p in want.reshape(-1, 3)}) >= (4 if only_mesh else 200)   # the frame shows the textured objects (the mesh: a few flat facets)
    options = ["coherent_waves", "classify_pixels", "uniform_surface"] + (["primary_mesh_kernel"] if only_mesh else [])
    try:
        base, _ = hip.render(cam, W, Hh, SPP, jit, seed=ft.DEFAULT_SEED)
        H.assert_frames_match(base, want, what=f"textured frame, {lights}, mesh {mesh}, mesh alone {only_mesh}")
        for values in itertools.product((1, 0), repeat=len(options)):   # every combination; all of them ship as 1
            for opt, v in zip(options, values):
                hip.set_option(opt, v)
            got, _ = hip.render(cam, W, Hh, SPP, jit, seed=ft.DEFAULT_SEED)
            assert np.array_equal(got, base), f"{dict(zip(options, values))} changes the textured frame ({lights}, mesh {mesh}, mesh alone {only_mesh})"
    finally:
        for opt in options:
            hip.set_option(opt, 1)


@pytest.mark.gpu
def test_aov_colour_plane_equals_closest(hip):
    """render_aov's colour plane against `closest` on the pixels' own sample rays (derived as tests/test_aov.py does), 32 x 24."""
    frame_scene(hip, "directional")
    w, h = 32, 24
    cam = ft.make_camera((0.5, 2.0, -5.5), (0.0, 0.0, 0.0), (0, 1, 0), H.deg(50.0), w / h)
    got = hip.render_aov(cam, w, h, 1, np.zeros((1, 2)), channels=["colour", "leaf"])
    pixels = [(x, y) for y in range(h) for x in range(w)]
    o, d = _pixel_rays(cam, w, h, pixels)
    hit, _, _, _, col = hip.closest(o + 1e-4 * d, d)                # slightOffset (Shading.fs:129)
    m = hit.reshape(h, w).astype(bool)
    assert np.array_equal(got["leaf"] >= 0, m) and m.sum() >= 300
    assert np.array_equal(got["colour"][m], col.reshape(h, w, 3)[m])
    assert len({tuple(c) for c in got["colour"][m]}) >= 10

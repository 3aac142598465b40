"""The shaders at their branch points, against a 60-digit restatement of Shading.fs.

group A   Vector.normalise through the specular term (black diffuse colour, shineyness 1: the colour is lightColour * (view^ . -reflected^)):
          |d| laddered across 1e-7 along each axis, |d| at 1e-150, 1e-160 (l2 subnormal), either side of l2 = 1e300, at 1e155 (l2 = inf), and
          lattice and generic directions at ordinary magnitudes, where the device's rsq + Newton reciprocal is not exact;
group B   the three routes of `**`: every exponent of tests/shading_tools.py (square-and-multiply, pow, black by rule, NaN), one tile each,
          under the bases 1, 1 - 2^-k, 0 +- 2^-k, 0, -0.5, -1 + 2^-k; B-inf: bases around 0 under an infinite light colour; 64 materials
          in one wavefront in several orders and alone;
group C   Oren-Nayar at its singular points: view, light and both along the normal, the light's elevation across the horizon and exactly in
          the surface's plane, the view's towards grazing, the azimuth at 0, pi/2 (laddered) and pi, |tangentLight| across 1e-7, nine
          roughnesses from 2^-1074 to 1e200, negative and NaN, and a light that is not white;
group D   visibility: an occluder laddered across the 1e-4 shadow offset with the normal towards and away from the ray, a blocker across a
          point light's distance (with the tie), the light over, under and on the offset origin, falloffs whose denominator is 0, negative
          or changes sign - through `colour_for_ray` and `blocked`;
group E   JitterFrame through soft lights, as frames against the oracle on the same streams: both sides of the 0.9 generator switch, the
          axes and the zero vector, scatter angles from 0 to beyond pi, 1, 4 and 255 samples; every sample direction of the one-sample
          frames replayed in mpmath, none within 1e-9 of a decision, so the occluded counts are exact; the depth of field at focal lengths
          0, 2^-30, 5 and 1e8 and apertures 0, 0.05 and pi/2, every sample's ray replayed and sent through colour_for_ray;
group F   the reflection weight: reflectance from 2^-1074 to inf, -0.0, -1 and NaN under one, two and three lights over an unlit plane and
          an open sky, the recursion limit at 0, 1 and 8, and a corridor of two facing planes;
group N   a hit normal that normalise returns unchanged (a plane under a scale of 2^24), through Oren-Nayar and its own reflection.

The expectation is the exact colour with a bound derived per case (tests/shading_tools.py); the CPU half holds the oracle to the same
bound, caps the rounding-decided cases at 10 % of a group and checks that every ladder keeps a case on each of its sides.  The device
answers through `colour_for_ray` (k_bounce) and through 16 x 8 frames at 1 and 4 samples of a zero jitter pattern (k_primary, its voted
path, k_primary_mesh, lean and FANCY) under every kernel-selecting option, which must all give the same bits.  Two measurements stand
beside the cases: the error of one `normalise` (oracle and device), and how close to Jitter.fs:31's 0.9 a binary64 normalise can be trusted.

Findings, the measured error-to-bound ratios and what is not covered: DESIGN.md §15.4."""
import functools
import itertools
import math
from collections import namedtuple

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from . import shading_tools as S

GROUPS = ["A", "B", "B-inf", "C", "D", "F", "N", "waves"]
MAX_ROUNDING_DECIDED = 0.10
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_traced", "hits_primary", "rays_reference_equivalent")


# =============================================================================================================================
# References, computed once per process and shared by the CPU and the GPU halves

@functools.lru_cache(maxsize=None)
def group(name):
    """(tile materials or None, cases, verdicts)."""
    if name == "A":
        mats, cases = None, S.group_a()
    elif name == "B":
        mats, cases = S.group_b()
    elif name == "B-inf":
        mats, cases = S.group_b_inf()
    elif name == "C":
        mats, cases = None, S.group_c()
    elif name == "D":
        mats, cases = None, S.group_d()
    elif name == "F":
        mats, cases = None, S.group_f()
    elif name == "N":
        mats, cases = None, S.group_n()
    else:
        mats = S.wave_materials()
        light = [(S.C_LIGHT, (1.0, 0.5, 0.25))]
        o, d = S.wave_rays(range(64))
        cases = [S.Case(f"tile {k}: {mats[k]}", list(o[k]), list(d[k]), mats[k], light, k) for k in range(64)]
    return mats, cases, [S.evaluate(c) for c in cases]


def colours(b, name):
    """colour_for_ray of every case of the group through builder b, scene by scene."""
    mats, cases, _ = group(name)
    if mats is not None:
        S.build_scene(b, mats, cases[0].lights, tiles=True)
        return b.colour_for_ray([c.o for c in cases], [c.d for c in cases])
    out = np.zeros((len(cases), 3))
    for mat, lights, idx in S.scenes_of(cases):
        S.build_scene(b, [mat], lights, above=cases[idx[0]].above, scale=cases[idx[0]].scale)
        out[idx] = b.colour_for_ray([cases[i].o for i in idx], [cases[i].d for i in idx], max_depth=cases[idx[0]].depth)
    return out


@functools.lru_cache(maxsize=None)
def oracle_colours(name):
    return colours(O.Oracle(), name)


def check_against_reference(got, name, who, capsys):
    """Kept cases: the class of every channel (NaN, +inf, -inf, finite) and the bound.  Cases at which C pow and Math.Pow differ, and
    rounding-decided ones (their verdict follows the oracle's branches): against the oracle, same class and the same bound."""
    _, cases, verdicts = group(name)
    orc = oracle_colours(name)
    worst, at = 0.0, None
    for c, v, g, w in zip(cases, verdicts, got, orc):
        if v.differs or not v.kept:
            assert S.classes(g) == S.classes(w), f"{who}, {c.name}: {list(g)}, the oracle {list(w)}"
            ok = all(abs(a - b) <= e for a, b, e in zip(g, w, v.bound) if math.isfinite(b))
            assert ok, f"{who}, {c.name}: {list(g)}, the oracle {list(w)}, bound {v.bound}"
            continue
        assert S.classes(g) == S.classes(v.colour), f"{who}, {c.name} (d = {c.d}): {list(g)}, exactly {v.colour}"
        r = S.error_ratio(g, v)
        if r > worst:
            worst, at = r, c.name
    with capsys.disabled():
        print(f"\n  group {name}, {who}: worst error / bound {worst:.3g} ({at})", end="")
    assert worst <= 1.0, f"{who}, group {name}: {at} is {worst:.3g} bounds from the exact colour"
    return worst


# =============================================================================================================================
# CPU half

def test_restatement_on_hand_worked_values():
    K = S.Exact()
    assert [float(c) for c in S.normalise(K, [K.num(3.0), K.num(4.0), K.num(0.0)], "v")] == [0.6, 0.8, 0.0]
    tiny = [K.num(6e-8), K.num(0.0), K.num(7.9e-8)]                   # |v| = 9.92e-8 < 1e-7: unchanged (CommonTypes.fs:65-66)
    assert S.normalise(K, tiny, "v") == tiny and K.branches == [("v: |v| < 1e-7", False), ("v: |v| < 1e-7", True)]
    assert [float(c) for c in S.normalise(K, [K.num(1e155), K.num(0.0), K.num(0.0)], "v")] == [0.0, 0.0, 0.0]       # l2 = inf, 1 / inf = 0
    assert [float(c) for c in S.reflect(K, [K.num(0.0), K.num(1.0), K.num(0.0)], [K.num(0.6), K.num(-0.8), K.num(0.0)])] == [0.6, 0.8, 0.0]
    inf, nan = S.INF, S.NAN
    for x, y, want in ((2.0, 3.0, 8.0), (-2.0, 3.0, -8.0), (-2.0, 2.0, 4.0), (-0.5, 2.5, nan), (0.0, 2.0, 0.0), (0.0, -1.0, inf), (0.5, inf, 0.0), (2.0, inf, inf),
                       (0.5, -inf, inf), (1.0, nan, 1.0), (1.0, inf, 1.0), (-1.0, inf, 1.0), (0.5, nan, nan), (0.5, 1e300, 0.0), (-0.5, 1e300, 0.0),
                       (1.0 - 2.0 ** -52, 1e300, 0.0), (0.5, 2.0 ** -1074, 1.0), (0.25, 0.5, 0.5), (4.0, 0.0, 1.0), (0.5, 1075.0, 0.0)):
        for A in (S.Exact(), S.Binary64()):
            got = float(A.pow(A.num(x), A.num(y)))
            assert (got != got and want != want) or got == want, (x, y, got, want, type(A).__name__)
    assert S.pow_differs(1.0, nan) and S.pow_differs(-1.0, inf) and S.pow_differs(1.0, -inf) and not S.pow_differs(0.5, nan) and not S.pow_differs(0.5, inf)
    # specular (Shading.fs:78-87): light straight down, view straight down: the base is 1
    n, down, lc = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.5, 0.25)
    shade = lambda mat, d=down, l=down: [float(c) for c in S.shade(S.Exact(), n, d, mat, [S.Light("directional", l, lc)])]
    assert shade(S.Material(shineyness=2.0)) == [1.0, 0.5, 0.25] and shade(S.Material(shineyness=-1.0)) == [0.0, 0.0, 0.0]
    assert shade(S.Material(shineyness=2.0), l=(0.0, 1.0, 0.0)) == [0.0, 0.0, 0.0]            # a light from under the plane: blocked, and base -1
    assert shade(S.Material(shineyness=3.0), d=(0.0, 1.0, 0.0)) == [0.0, 0.0, 0.0]            # base -1, cubed: negative, black
    assert all(c != c for c in shade(S.Material(shineyness=nan), d=(0.6, -0.8, 0.0)))          # 0.8 ** nan
    assert shade(S.Material((0.5, 0.25, 1.0))) == [0.5, 0.125, 0.25]                          # lambertian: 1 * (colour * lightColour)
    # Oren-Nayar with both angles 0 (Shading.fs:50-63): cos 0 * (A + B * 0 * sin 0 * tan 0) = A = 1 - 0.5 * 0.25 / 0.58
    got = shade(S.Material((1.0, 0.5, 0.0), 0.5))
    assert np.allclose(got, [1.0 - 0.125 / 0.58, 0.5 * (1.0 - 0.125 / 0.58), 0.0], rtol=1e-15, atol=0)
    assert all(c != c for c in shade(S.Material((1.0, 0.5, 0.25), 1e200)))                     # r^2 = inf: A = 1 - inf / inf


@pytest.mark.parametrize("name", GROUPS)
def test_closed_forms_hold_on_oracle(name):
    """The hit, its normal, the light's stored direction and the shadow ray's verdict, as tests/shading_tools.py takes them for granted."""
    mats, cases, _ = group(name)
    orc = O.Oracle()
    scenes = [(None, cases[0].lights, list(range(len(cases))))] if mats is not None else S.scenes_of(cases)
    for mat, lights, idx in scenes:
        S.build_scene(orc, mats if mats is not None else [mat], lights, tiles=mats is not None, above=cases[idx[0]].above, scale=cases[idx[0]].scale)
        o = np.array([[a + 0.0001 * b for a, b in zip(cases[i].o, cases[i].d)] for i in idx])      # slightOffset (Shading.fs:129)
        d = np.array([cases[i].d for i in idx])
        hit, t, p, n, _ = orc.closest(o, d)
        for k, i in enumerate(idx):
            want, at_origin = S.plane_hit(cases[i].o, cases[i].d, cases[i].scale)
            assert want and hit[k], f"{cases[i].name}: every case is a hit"
            assert tuple(n[k]) == tuple(cases[i].n) and (not at_origin or (t[k] == 0.0 and tuple(p[k]) == tuple(o[k]))), cases[i].name
            if mats is not None:
                x, _, z = S.tile_centre(cases[i].tile)
                assert abs(p[k][0] - x) < 0.25 and abs(p[k][2] - z) < 0.25 and abs(p[k][1]) < 1.0, f"{cases[i].name}: the hit {p[k]} is off its tile"
            if name in ("D", "F"):                                  # the receiver's point: (0, 0, 0), the height exactly
                assert p[k][1] == 0.0 and abs(p[k][0]) <= 2.0 ** -30 and p[k][2] == 0.0, f"{cases[i].name}: the hit is {p[k]}"
        if name in ("D", "F"):
            continue                                                # (D's shadow rays: test_blocked_on_oracle; F's lights are open or in group D's forms)
        for direction in [S.stored_direction(l.v) for l in S.as_lights(lights)]:
            shadow_o = p + 0.0001 * n
            got = orc.blocked(shadow_o, np.tile([-c for c in direction], (len(idx), 1)), np.full(len(idx), 1.7976931348623157e308))
            assert (got != 0).all() == S.plane_blocked([c / cases[idx[0]].scale for c in direction]) and len(set(got)) == 1, f"light {direction}: blocked {set(got)}"
    # the stored direction: a white lambertian plane's colour is -direction.y
    for direction in {l.v for c in cases for l in S.as_lights(c.lights) if l.kind == "directional" and not S.plane_blocked(S.stored_direction(l.v))}:
        S.build_scene(orc, [S.Material((1.0, 1.0, 1.0))], [(direction, (1.0, 1.0, 1.0))])
        assert orc.colour_for_ray([[0.0, 1.0, 0.0]], [[0.0, -1.0, 0.0]])[0][0] == -S.stored_direction(direction)[1], direction


def check_blocked(b, who):
    """`blocked` on the shadow ray of every light of group D, from the offset origin over (0, 0, 0): the closed form, exactly."""
    _, cases, verdicts = group("D")
    for mat, lights, idx in S.scenes_of(cases):
        S.build_scene(b, [mat], lights)
        o, d, far = S.shadow_query(S.as_lights(lights)[0])
        got = bool(b.blocked([o], [d], [far])[0])
        v = verdicts[idx[0]]
        assert not v.kept or got == S.in_the_way(v), f"{who}, {cases[idx[0]].name}: blocked is {got} from {o} along {d} up to {far}"


def test_blocked_on_oracle():
    check_blocked(O.Oracle(), "oracle")


@pytest.mark.parametrize("name", GROUPS)
def test_group_caps_ladders_and_oracle(name, capsys):
    _, cases, verdicts = group(name)
    undecided = sum(not v.kept for v in verdicts)
    assert undecided <= MAX_ROUNDING_DECIDED * len(cases), f"group {name}: {undecided} of {len(cases)} cases are rounding-decided"
    ladders = {}
    for c, v in zip(cases, verdicts):
        if c.ladder:
            ladders.setdefault(c.ladder, []).append((c, v))
    assert name in ("waves", "B-inf", "F", "N") or len(ladders) >= 3
    for ladder, rungs in ladders.items():
        built = {c.side for c, _ in rungs if c.side}
        kept = {c.side for c, v in rungs if c.side and v.kept and not v.differs}
        assert built and kept == built, f"{ladder}: kept rungs on sides {kept} of {built}"
        watch = {c.watch for c, _ in rungs}
        assert len(watch) == 1
        if None not in watch and {1, -1} <= built:                 # a ladder across a decision: both outcomes among the kept rungs
            taken = {dict(v.branches)[c.watch] for c, v in rungs if v.kept}
            assert taken == {True, False}, f"{ladder}: {c.watch} is only ever {taken}"
    with capsys.disabled():
        print(f"\n  group {name}: {len(cases)} cases, {len(ladders)} ladders, {undecided} rounding-decided, {sum(v.differs for v in verdicts)} where C pow and Math.Pow differ", end="")
    check_against_reference(oracle_colours(name), name, "oracle", capsys)


def test_group_shapes():
    """What the catalogue of DESIGN.md §15.4 promises about the groups."""
    _, a, va = group("A")
    ladder = [v for c, v in zip(a, va) if c.ladder == "|d| across 1e-7 along -x"]
    assert any(abs(v.colour[0]) < 1e-6 for v in ladder) and any(abs(v.colour[0]) > 0.1 for v in ladder)   # unchanged: 1e-7 * base; unit: base
    assert [v.colour for c, v in zip(a, va) if "1e+155" in c.name] == [[0.0, 0.0, 0.0]] * 3
    mats, b, vb = group("B")
    assert len(mats) == len(S.EXPONENTS) == 21 and len(b) == 21 * 31
    near_one = {v.base for c, v in zip(b, vb) if c.name.startswith("base 1 - ")}
    assert len(near_one) == len(S.K_FEW) and all(0.0 < 1.0 - x < 2.0 ** -9 for x in near_one) and min(1.0 - x for x in near_one) < 2.0 ** -51
    assert {v.base for c, v in zip(b, vb) if c.name.startswith("base 1 **")} == {1.0} and {v.base for c, v in zip(b, vb) if c.name.startswith("base 0 **")} == {0.0}
    assert sum(v.differs for v in vb) == 3                         # 1 ** inf, 1 ** -inf, 1 ** nan: the lattice holds no base of exactly -1
    nan_cases = [v for c, v in zip(b, vb) if c.mat.shineyness != c.mat.shineyness and not v.differs]
    assert len(nan_cases) == 30 and all(S.classes(v.colour) == ["nan"] * 3 for v in nan_cases)              # x ** nan is NaN and not <= 0
    _, c, vc = group("C")
    horizon = [(k.side, v) for k, v in zip(c, vc) if k.ladder == "light elevation across the horizon"]
    assert all(v.colour[0] * side > 0 for side, v in horizon if side)                                      # cos lightAngle changes sign
    tl = [(dict(v.branches)["tangentLight: |v| < 1e-7"], v.colour[0]) for k, v in zip(c, vc) if k.ladder == "|tangentLight| across 1e-7"]
    assert max(x for small, x in tl if not small) - min(x for small, x in tl if not small) < 1e-9
    assert all(S.classes(v.colour) == ["nan"] * 3 for k, v in zip(c, vc) if "roughness 1e+200" in k.name or "roughness nan" in k.name)
    _, d, vd = group("D")
    over = {c.name: v.colour for c, v in zip(d, vd) if c.ladder and c.ladder.startswith("the light over the offset origin, falloff (0.0, 0.0, 1.0)")}
    rung = lambda name: int(name.split("2^-")[1].split(",")[0])
    assert len(over) == 10 and all(math.isclose(v[0], 4.0 ** rung(k), rel_tol=1e-6) if rung(k) <= 23 else v[0] == 0.0 for k, v in over.items())   # 1 / dist^2, or the parallel rule
    zero = [v.colour for c, v in zip(d, vd) if "falloff (0.0, 0.0, 0.0)" in c.name and S.in_the_way(v) is False]
    assert len(zero) == 10 and all(S.classes(c) == ["+inf", "+inf", "nan"] for c in zero)                   # 1 / 0 = inf, inf * 0 = NaN
    under = [v.colour for c, v in zip(d, vd) if "1e-4 - 2^-20, falloff (-1.0, 0.0, 0.0)" in c.name]
    assert under == [[-1.0, -0.5, 0.0]]                            # L from p says "above", the distance from p + 1e-4 n says 2^-20 "below": lit, by -1
    _, w, vw = group("waves")
    assert len({(m.roughness, repr(m.shineyness)) for m in S.wave_materials()}) == 64


def normalise_error(b):
    """The worst relative error, in units of 2^-53, of a unit sphere's normal n = normalise(p) (Sphere.fs) against p / |p| at 60 digits, p
    being the hit point the builder itself reports: `closest` hands out one normalisation's input and output."""
    import mpmath
    H.single_prim(b, "sphere")
    o, d = H.random_rays(2000, seed=3, origin_scale=3.0, toward=(0, 0, 0), spread=0.5)
    hit, _, p, n, _ = b.closest(o, d)
    assert hit.sum() >= 1500
    worst = 0.0
    for k in np.nonzero(hit)[0]:
        pv = [mpmath.mpf(float(c)) for c in p[k]]
        l = mpmath.sqrt(sum(c * c for c in pv))
        worst = max([worst] + [float(abs(mpmath.mpf(float(n[k][c])) * l / pv[c] - 1) * 2 ** 53) for c in range(3) if abs(p[k][c]) > 1e-3])
    return worst


NORMALISE_UNITS = 4.0                                               # the perturbation the bounds are built from (shading_tools.ULPS); DESIGN.md 3 claims "an ulp or two"


def test_normalise_error_on_oracle(capsys):
    worst = normalise_error(O.Oracle())
    with capsys.disabled():
        print(f"\n  normalise, oracle (sqrt, divide): worst relative error {worst:.2f} x 2^-53", end="")
    assert worst <= NORMALISE_UNITS


class CMaxMin:
    """C's fmax and fmin, which drop a NaN, in place of F#'s max and min, which return it - in the Oren-Nayar angles and nowhere else."""
    def fmax(self, a, b): return b if a != a else (a if b != b else (b if a < b else a))
    def fmin(self, a, b): return b if a != a else (a if b != b else (a if a < b else b))


def test_what_a_nan_angle_can_show():
    """Shading.fs:56-57 take max and min of the two angles, and F#'s propagate a NaN where C's fmax and fmin would not.  What that can
    show: (1) an angle that is NaN because a direction or the normal is not finite takes the colour with it either way - the same vector
    goes into tangentRay or tangentLight, into `max 0.0` and into cos lightAngle - so no such input tells the two apart; (2) it shows only
    when a dot product of two unit vectors ROUNDS past 1, which the oracle's sqrt-and-divide and the device's rsq-and-Newton need not do
    on the same ray: a difference no test can pin on both sides."""
    nan, inf = S.NAN, S.INF
    n, light = (0.0, 1.0, 0.0), [S.Light("directional", S.stored_direction(S.C_LIGHT), S.WHITE)]
    odd = [((nan, -1.0, 0.0), n, light), ((inf, -1.0, 0.0), n, light), ((0.0, -inf, 0.0), n, light), ((0.3, -1.0, 0.2), (nan, 1.0, 0.0), light), ((0.3, -1.0, 0.2), (0.0, inf, 0.0), light),
           ((0.3, -1.0, 0.2), n, [S.Light("directional", (nan, -0.0, 0.0), S.WHITE)]), ((0.3, -1.0, 0.2), n, [S.Light("directional", (-0.6, nan, 0.8), S.WHITE)])]
    for base in (S.Binary64, S.Exact):
        c_rules = type("C" + base.__name__, (CMaxMin, base), {})
        assert float(base().fmax(base().num(nan), base().num(0.3))) != float(base().fmax(base().num(nan), base().num(0.3))) and float(c_rules().fmax(c_rules().num(nan), c_rules().num(0.3))) == 0.3
        for d, normal, lights in odd:
            fs = [float(c) for c in S.shade(base(), normal, d, S.ROUGH, lights)]
            c = [float(c) for c in S.shade(c_rules(), normal, d, S.ROUGH, lights)]
            assert S.classes(fs) == ["nan"] * 3 == S.classes(c), (base.__name__, d, normal, fs, c)
    # (2): the view along a slanted normal whose self dot product rounds to 1 + 2^-52 in binary64
    rng = np.random.default_rng(11)
    for _ in range(4000):
        v = S.normalise(S.Binary64(), [float(x) for x in rng.normal(size=3)], "v")
        if S.Binary64().dot(v, v) > 1.0:
            break
    fs = [float(c) for c in S.shade(S.Binary64(), v, [-x for x in v], S.ROUGH, light)]
    c = [float(c) for c in S.shade(type("C", (CMaxMin, S.Binary64), {})(), v, [-x for x in v], S.ROUGH, light)]
    exact = [float(x) for x in S.shade(S.Exact(), v, [-x for x in v], S.ROUGH, light)]
    assert S.classes(fs) == ["nan"] * 3 and S.classes(c) == ["finite"] * 3 == S.classes(exact)


def test_generator_switch_band(capsys):
    """Jitter.fs:31 reads `normalised.x > 0.9`.  Within this band of 0.9 a binary64 normalise and the exact one choose different generators:
    there the sample stream of a soft light or of the depth of field may differ between two correct implementations (its distribution does
    not).  The bound: the relative error of (1 / sqrt(x^2 + y^2 + z^2)) * x in binary64 - three roundings in the sum of squares, halved by
    the root, the root's, the reciprocal's and the product's: under 3 * 2^-53 - at x^ = 0.9, with one more unit for the comparison's side."""
    widest, flips = S.generator_band()
    with capsys.disabled():
        print(f"\n  0.9 switch: binary64 and exact normalise disagree on {flips} of 100000 directions within 8 units of it, the widest {widest:.3e} = {widest / 2.0 ** -53:.2f} x 2^-53 away", end="")
    assert flips > 1000 and widest <= 4.0 * 2.0 ** -53


# =============================================================================================================================
# GPU half

@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUPS)
def test_groups_on_device(hip, name, capsys):
    check_against_reference(colours(hip, name), name, "device", capsys)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_normalise_error_on_device(hip, capsys):
    """1 / |v| from v_rsq_f64 and two Newton steps, measured."""
    worst = normalise_error(hip)
    with capsys.disabled():
        print(f"\n  normalise, device (rsq, two Newton steps): worst relative error {worst:.2f} x 2^-53", end="")
    assert worst <= NORMALISE_UNITS


@pytest.mark.gpu
def test_blocked_on_device(hip):
    check_blocked(hip, "device")


@pytest.mark.gpu
def test_mixed_waves_on_device(hip):
    """64 consecutive rays onto 64 materials: every ray's colour has the bits of the same ray sent alone, in any order and company
    (shade_lights: "a ray's result must not depend on its wave")."""
    mats, cases, _ = group("waves")
    S.build_scene(hip, mats, cases[0].lights, tiles=True)
    o, d = S.wave_rays(range(64))
    alone = np.concatenate([hip.colour_for_ray(o[k:k + 1], d[k:k + 1]) for k in range(64)])
    distinct = len({tuple("nan" if c != c else round(c, 9) for c in v.colour) for v in group("waves")[2]})
    assert distinct >= 20 and len({tuple(c) for c in bits(alone)}) >= distinct          # the wave is mixed: as many colours as the exact ones
    rng = np.random.default_rng(5)
    orders = [np.arange(64), np.arange(64)[::-1], rng.permutation(64), rng.permutation(64), np.arange(1), np.arange(63), np.arange(65) % 64,
              np.repeat(np.arange(64), 2), rng.permutation(np.arange(192) % 64)]
    for order in orders:
        got = hip.colour_for_ray(o[order], d[order])
        bad = np.nonzero((bits(got) != bits(alone[order])).any(axis=1))[0]
        assert bad.size == 0, f"{len(order)} rays: rays {bad[:6]} (tiles {order[bad[:6]]}) differ from the same rays alone: {got[bad[:2]]} vs {alone[order][bad[:2]]}"


# ---- frames: every instance of the shader ----------------------------------------------------------------------------------------

W, Hh = 16, 8
def quad_mesh():
    """The plane's stand-in as a mesh: [-9, 40]^2 at y = 0 as 2 x 2 cells of two triangles, every normal (0, 1, 0) - eight triangles, the
    fewest that get a BVH.  The frame looks at the first cell, and no pixel centre's point lies on an edge (x + z = 6.3 is its diagonal)."""
    cuts = (-9.0, 15.3, 40.0)
    tris = []
    for (x0, x1), (z0, z1) in itertools.product(zip(cuts, cuts[1:]), repeat=2):
        tris += [[x0, 0.0, z0, x0, 0.0, z1, x1, 0.0, z0], [x1, 0.0, z1, x1, 0.0, z0, x0, 0.0, z1]]
    return np.array(tris)


GENERIC_LIGHT = [((1.0, -2.0, 2.0), (1.0, 0.5, 0.25))]
DOWN_LIGHT = [((0.0, -1.0, 0.0), (1.0, 0.5, 0.25))]
LEAN_MATS = [S.Material((0.8, 0.6, 0.4), 0.0, 0.0, e) for e in S.LEAN_EXPONENTS]
ALL_MATS = [S.Material((0.8, 0.6, 0.4), 0.0, 0.0, e) for e in S.EXPONENTS]
ROUGH_MATS = [S.Material(S.C_COLOUR, r, 0.0, 2.0) for r in S.ROUGHNESSES]
E7 = S.EPS
# tile materials or the plane's one; lights; FANCY by a far rough sphere; an eight-triangle mesh as receiver; what lies above (shading_tools.Case);
# the recursion limit; the camera: "high" (100 over the plane), "low" (1.5 over it, under what lies above) or "under" (100 under the plane, whose
# normal then points away from every pixel ray); whether pixels are held to the restatement (not where the colour depends on an inexact p)
FrameScene = namedtuple("FrameScene", "mats lights fancy mesh above depth camera designate", defaults=(False, False, None, 8, "high", True))
F_FLOOR = lambda r: [S.Material(S.F_COLOUR, 0.0, r, 0.0)]
LAMP = S.Light("point", (0.0, 1.0, 0.0), (0.8, 0.6, 0.4), (1.0, 0.0, 0.0))
HIGH_LAMP = S.exact_height(2.0)
FRAME_SCENES = {
    "A: shineyness 1 over black, lean": ([S.SHINE_ONE], [S.A_LIGHT]),
    "A: shineyness 1 over black, FANCY": ([S.SHINE_ONE], [S.A_LIGHT], True),
    "D: occluder 2^-20 under the offset origin": ([S.D_WHITE], [S.Light("directional", (0.0, -1.0, 0.0), S.D_COLOUR, occluder=S.OFFSET * (1.0 - 2.0 ** -20))], False, False, None, 8, "under"),
    "D: occluder at the offset origin": ([S.D_WHITE], [S.Light("directional", (0.0, -1.0, 0.0), S.D_COLOUR, occluder=S.OFFSET)], False, False, None, 8, "under"),
    "D: occluder 2^-20 over the offset origin": ([S.D_WHITE], [S.Light("directional", (0.0, -1.0, 0.0), S.D_COLOUR, occluder=S.OFFSET * (1.0 + 2.0 ** -20))], False, False, None, 8, "under"),
    "D: blocker just under a point light": ([S.D_WHITE], [S.Light("point", (0.0, HIGH_LAMP, 0.0), S.D_COLOUR, (0.0, 0.0, 1.0), HIGH_LAMP * (1.0 - 2.0 ** -20))], False, False, None, 8, "under"),
    "D: blocker just over a point light": ([S.D_WHITE], [S.Light("point", (0.0, HIGH_LAMP, 0.0), S.D_COLOUR, (0.0, 0.0, 1.0), HIGH_LAMP * (1.0 + 2.0 ** -20))], False, False, None, 8, "under"),
    "D: point light 2^-20 over the offset origin, falloff 0": ([S.D_WHITE], [S.Light("point", (0.0, S.OFFSET + 2.0 ** -20, 0.0), (1.0, 0.5, 0.0), (0.0, 0.0, 0.0))], False, False, None, 8, "under"),
    "D: point light 2^-20 under the offset origin, falloff -1": ([S.D_WHITE], [S.Light("point", (0.0, S.OFFSET - 2.0 ** -20, 0.0), (1.0, 0.5, 0.0), (-1.0, 0.0, 0.0))], False, False, None, 8, "under"),
    "F: reflectance 2 under an unlit plane, three lights": (F_FLOOR(2.0), S.F_LIGHTS, False, False, ("unlit", S.F_SEEN), 8, "low"),
    "F: reflectance 1 under an unlit plane, two lights, depth 0": (F_FLOOR(1.0), S.F_LIGHTS[:2], False, False, ("unlit", S.F_SEEN), 0, "low"),
    "F: reflectance inf under an unlit plane, depth 1": (F_FLOOR(S.INF), S.F_LIGHTS[:1], False, False, ("unlit", S.F_SEEN), 1, "low"),
    "F: reflectance inf under an open sky": (F_FLOOR(S.INF), S.F_LIGHTS[:2]),
    "F: reflectance nan under an unlit plane": (F_FLOOR(S.NAN), S.F_LIGHTS, False, False, ("unlit", S.F_SEEN), 8, "low"),
    "F: two facing planes, depth 8": (F_FLOOR(0.5), [LAMP], False, False, ("mirror",), 8, "low", False),
    "F: two facing planes, depth 1": (F_FLOOR(0.5), [LAMP], False, False, ("mirror",), 1, "low", False),
    "exponents, lean": (LEAN_MATS, GENERIC_LIGHT, False, False),
    "exponents, lean materials in the FANCY kernels": (LEAN_MATS, GENERIC_LIGHT, True, False),
    "exponents, all": (ALL_MATS, GENERIC_LIGHT, False, False),
    "exponents, all, light straight down": (ALL_MATS, DOWN_LIGHT, False, False),
    "32 materials": (S.wave_materials()[:32], GENERIC_LIGHT, False, False),
    "roughnesses": (ROUGH_MATS, GENERIC_LIGHT, False, False),
    "rough, light along the normal": ([S.ROUGH], DOWN_LIGHT, False, False),
    "rough, light in the plane": ([S.ROUGH], [((-1.0, 0.0, 0.0), S.WHITE)], False, False),
    "rough, light 2^-30 above the horizon": ([S.ROUGH], [((-1.0, -2.0 ** -30, 0.0), S.WHITE)], False, False),
    "rough, light 2^-12 above the horizon": ([S.ROUGH], [((-1.0, -2.0 ** -12, 0.0), S.WHITE)], False, False),
    "rough, light 2^-12 below the horizon": ([S.ROUGH], [((-1.0, 2.0 ** -12, 0.0), S.WHITE)], False, False),
    "rough, |tangentLight| under 1e-7": ([S.ROUGH], [((-E7 * (1.0 - 2.0 ** -20), -1.0, 0.0), S.WHITE)], False, False),
    "rough, |tangentLight| over 1e-7": ([S.ROUGH], [((-E7 * (1.0 + 2.0 ** -20), -1.0, 0.0), S.WHITE)], False, False),
    "shiny plane, two lights, lean": ([S.Material((0.8, 0.6, 0.4), 0.0, 0.0, 64.0)], GENERIC_LIGHT + DOWN_LIGHT, False, False),
    "shiny plane, two lights, FANCY": ([S.Material((0.8, 0.6, 0.4), 0.0, 0.0, 64.0)], GENERIC_LIGHT + DOWN_LIGHT, True, False),
    "mesh, exponent 1": ([S.Material((0.8, 0.6, 0.4), 0.0, 0.0, 1.0)], GENERIC_LIGHT, False, True),
    "mesh, exponent 3": ([S.Material((0.8, 0.6, 0.4), 0.0, 0.0, 3.0)], GENERIC_LIGHT + DOWN_LIGHT, False, True),
    "mesh, exponent 64": ([S.Material((0.8, 0.6, 0.4), 0.0, 0.0, 64.0)], DOWN_LIGHT, False, True),
    "mesh, exponent -0.0": ([S.Material((0.8, 0.6, 0.4), 0.0, 0.0, -0.0)], GENERIC_LIGHT, False, True),
}
FRAME_SCENES = {name: FrameScene(*scene) for name, scene in FRAME_SCENES.items()}


def build_frame_scene(b, name):
    mats, lights, fancy, mesh, above = FRAME_SCENES[name][:5]
    if not mesh:
        return S.build_scene(b, mats, lights, tiles=len(mats) > 1, fancy=fancy, above=above)
    m = mats[0]
    b.clear()
    b.set_objects(b.group([b.material(b.bsp_mesh(0, quad_mesh()), colour=m.colour, roughness=m.roughness, reflectance=m.reflectance, shineyness=m.shineyness)]))
    for direction, colour in lights:
        b.add_directional(direction, colour)
    b.commit()


def frame_camera(name):
    """Straight down from 100 above the plane y = 0, the image plane sized so that a pixel is a unit of the plane (Image.fs:69-72 and 80
    divide the height by resH - 1 and the width by resV - 1, and start half a pixel in): pixel (px, py) looks at x = px - 0.5,
    z = 6.5 - py - every other one the centre of a tile (eight across, four rows), the rest between the tiles."""
    kind = FRAME_SCENES[name].camera
    if kind == "under":                                             # the pixel centres on the integer lattice: one of them looks at (0, 0, 0) from below
        return ft.make_camera((3.0, -100.0, 0.0), (3.0, 0.0, 0.0), (0, 0, 1), 2.0 * math.atan(0.075), 0.07 / 0.15)
    return ft.make_camera((2.5, 100.0 if kind == "high" else 1.5, -0.5), (2.5, 0.0, -0.5), (0, 0, 1), 2.0 * math.atan(0.075), 0.07 / 0.15)


@functools.lru_cache(maxsize=None)
def frame_reference(name):
    """Per pixel: the centre ray, and for a designated pixel (its ray meets the plane y = 0 at least 0.05 inside a tile, or anywhere on a
    plane or the quad) the material it meets and the verdict of tests/shading_tools.py."""
    scene = FRAME_SCENES[name]
    mats, lights = scene.mats, scene.lights
    cam = frame_camera(name)
    out = []
    for y, x in itertools.product(range(Hh), range(W)):
        o, d = O.ray_through_pixel(cam, W, Hh, x, y)
        hit, _ = S.plane_hit(o, d)
        mat = None
        if hit and abs(d[1]) > 1e-3 and scene.designate:
            t = -o[1] / d[1]
            px, pz = o[0] + t * d[0], o[2] + t * d[2]
            if scene.camera == "under":                             # the one pixel that looks at the receiver's point of group D
                mat = mats[0] if (abs(px) < 0.25 and abs(pz) < 0.25) else None
            elif len(mats) == 1:
                mat = mats[0] if (x % 4 == 1 and y % 2 == 1) else None                 # sixteen of the pixels of a plane or the quad
            else:
                i, j = math.floor(px / S.TILE_STEP), math.floor(pz / S.TILE_STEP)
                fx, fz = px - S.TILE_STEP * i, pz - S.TILE_STEP * j
                if 0 <= i < 8 and j >= 0 and 8 * j + i < len(mats) and 0.05 < fx < 0.95 and 0.05 < fz < 0.95:
                    mat = mats[8 * j + i]
        verdict = S.evaluate(S.Case(f"pixel ({x}, {y})", list(o), list(d), mat, lights, above=scene.above, depth=scene.depth)) if mat is not None else None
        out.append(((x, y), o, d, mat, verdict))
    return out


def check_frame_pixels(frame, name, who, rays=None):
    """Designated pixels against the exact colour: class and bound (and the class of colour_for_ray of the same ray, given as `rays`)."""
    ref = frame_reference(name)
    designated = [r for r in ref if r[4] is not None]
    scene = FRAME_SCENES[name]
    mats = scene.mats
    want = 0 if not scene.designate else 1 if scene.camera == "under" else len(mats) if len(mats) > 1 else 16
    assert len(designated) == want, f"{name}: {len(designated)} designated pixels"
    worst = 0.0
    for k, ((x, y), _, _, mat, v) in enumerate(ref):
        if v is None:
            continue
        got = frame[y, x]
        if v.differs or not v.kept:
            continue                                                # (compared with the oracle's frame by the caller)
        assert S.classes(got) == S.classes(v.colour), f"{who}, {name}, pixel ({x}, {y}), {mat}: {list(got)}, exactly {v.colour}"
        if rays is not None:
            assert S.classes(got) == S.classes(rays[k]), f"{who}, {name}, pixel ({x}, {y}): {list(got)}, colour_for_ray {list(rays[k])}"
        worst = max(worst, S.error_ratio(got, v))
        assert worst <= 1.0, f"{who}, {name}, pixel ({x}, {y}), {mat}: {list(got)} is {worst:.3g} bounds from {v.colour}"
    return worst, len(designated)


@pytest.mark.parametrize("name", list(FRAME_SCENES))
def test_frame_pixels_on_oracle(name, capsys):
    orc = O.Oracle()
    build_frame_scene(orc, name)
    frame, _ = orc.render(frame_camera(name), W, Hh, 1, np.zeros((1, 2)), max_depth=FRAME_SCENES[name].depth)
    worst, n = check_frame_pixels(frame, name, "oracle")
    mats = FRAME_SCENES[name][0]
    if len(mats) > 1:
        met = {repr(r[3]) for r in frame_reference(name) if r[3] is not None}
        assert len(met) == len(mats), f"{name}: the designated pixels meet {len(met)} of {len(mats)} materials"
    with capsys.disabled():
        print(f"\n  {name}: {n} designated pixels, oracle worst error / bound {worst:.3g}", end="")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FRAME_SCENES))
def test_frames_under_every_option(hip, name, capsys):
    """k_primary, its voted path, k_primary_mesh's one-leaf path, lean and FANCY, and k_bounce on the same points."""
    mesh, depth = FRAME_SCENES[name].mesh, FRAME_SCENES[name].depth
    orc = O.Oracle()
    for b in (orc, hip):
        build_frame_scene(b, name)
    cam = frame_camera(name)
    ref = frame_reference(name)
    rays = hip.colour_for_ray([r[1] for r in ref], [r[2] for r in ref], max_depth=depth)
    options = {"uniform_surface": (1, 0), "coherent_waves": (1, 0), "wave_samples": (1, 4, 16)}
    if mesh:
        options["primary_mesh_kernel"] = (1, 0)
    worst = 0.0
    try:
        for spp in (1, 4):
            jit = np.zeros((spp, 2))
            want, ost = orc.render(cam, W, Hh, spp, jit, max_depth=depth)
            base, st0, launches = None, None, 0
            for values in itertools.product(*options.values()):
                for opt, v in zip(options, values):
                    hip.set_option(opt, v)
                before = hip.primary_kernels()["k_primary_mesh"]
                got, st = hip.render(cam, W, Hh, spp, jit, max_depth=depth)
                launches += hip.primary_kernels()["k_primary_mesh"] - before
                if base is None:
                    base, st0 = got, st
                    assert np.array_equal(np.isnan(base), np.isnan(want)) and np.array_equal(np.isinf(base), np.isinf(want)), f"{name}: NaN or inf pixels differ from the oracle's"
                    H.assert_frames_match(base, want, what=f"{name}, {spp} samples")
                    assert st["rays_reference_equivalent"] == ost["rays_traced"] and st["csg_overflow"] == 0
                    worst = max(worst, check_frame_pixels(base, name, "device", rays)[0])
                    for k, (_, _, _, _, v) in enumerate(ref):       # a pixel is its ray's colour: one sample, or four equal ones
                        if v is not None and v.kept and all(math.isfinite(c) for c in v.colour):
                            x, y = ref[k][0]
                            assert all(abs(a - b) <= 2.0 * e for a, b, e in zip(base[y, x], rays[k], v.bound)), f"{name}, pixel ({x}, {y}): the frame {base[y, x]}, colour_for_ray {rays[k]}"
                assert np.array_equal(bits(got), bits(base)), f"{name}, {spp} samples: {dict(zip(options, values))} changes the frame"
                assert all(st[k] == st0[k] for k in COUNTERS), f"{name}, {spp} samples: {dict(zip(options, values))} changes the counters: {st} vs {st0}"
            # k_primary_mesh takes frames in grouped numbering only (ft_frame.cpp: two or more samples of a pixel in a wavefront, which an
            # odd sample count does not allow): at one sample every launch is k_primary's, at four it must have run
            assert launches == 0 if (not mesh or spp == 1) else launches > 0, f"{name}, {spp} samples: {launches} launches of k_primary_mesh"
    finally:
        hip.set_option("wave_samples", 0)
        for opt in ("uniform_surface", "coherent_waves", "primary_mesh_kernel"):
            hip.set_option(opt, 1)
    with capsys.disabled():
        print(f"\n  {name}: device worst error / bound {worst:.3g}", end="")


# ---- soft lights: the generator switch, scatter angles and sample counts, through frames ---------------------------------------------

_UP, _DN = 0.9 + 2.0 ** -31, 0.9 - 2.0 ** -31                         # either side of Jitter.fs:31's 0.9, ten million band widths away
# Shading.fs:27 jitters -direction: it is the light's direction with x^ = -0.9 whose frame is built around x^ = +0.9
_AT = (-0.9, -math.sqrt(0.19), 0.0)
_TOWARDS = lambda x: (-x, -math.sqrt(1.0 - x * x), 0.0)
_DOWN = (0.0, -1.0, 0.0)
_WIDE = math.radians(20.0)
# name -> (direction, samples, scatter angle)
SOFT_CASES = {
    "x^ = 0.9 + 2^-31": (_TOWARDS(_UP), 4, _WIDE), "x^ = 0.9 - 2^-31": (_TOWARDS(_DN), 4, _WIDE), "x^ = 0.9 + 2^-31, 255 samples": (_TOWARDS(_UP), 255, _WIDE),
    "x^ = 0.9 - 2^-31, 1 sample": (_TOWARDS(_DN), 1, _WIDE), "-(0.9, sqrt 0.19, 0) rounded, scatter 0": (_AT, 4, 0.0), "down, scatter 0": (_DOWN, 4, 0.0),
    "down, scatter 0, 255 samples": (_DOWN, 255, 0.0), "down, scatter 2^-1074": (_DOWN, 4, 2.0 ** -1074), "down, scatter 1e-8": (_DOWN, 4, 1e-8),
    "down, scatter pi/2": (_DOWN, 4, math.pi / 2.0), "down, scatter pi - 2^-20": (_DOWN, 4, math.pi - 2.0 ** -20), "down, scatter 3.5": (_DOWN, 4, 3.5),
    "(0, 0, 1)": ((0.0, 0.0, 1.0), 4, _WIDE), "(-1, 0, 0)": ((-1.0, 0.0, 0.0), 4, _WIDE), "(1, 0, 0)": ((1.0, 0.0, 0.0), 4, _WIDE), "(0, 1, 0)": ((0.0, 1.0, 0.0), 4, _WIDE),
    "the zero vector": ((0.0, 0.0, 0.0), 4, _WIDE),
}


def soft_scene(b, direction, samples, scatter, soft=True):
    """A white plane under a sphere of radius 2 at (5, 3, 3), one light."""
    b.clear()
    ball = b.transform([("scale", (2.0, 2.0, 2.0)), ("translate", (5.0, 3.0, 3.0))], b.primitive(ft.SPHERE))
    b.set_objects(b.group([b.material(b.primitive(ft.PLANE), colour=(1, 1, 1)), b.material(ball, colour=(1, 1, 1))]))
    if soft:
        b.add_soft_directional(direction, samples, scatter, S.D_COLOUR)
    else:
        b.add_directional(direction, S.D_COLOUR)
    b.commit()


@functools.lru_cache(maxsize=None)
def soft_oracle(name, spp):
    orc = O.Oracle()
    soft_scene(orc, *SOFT_CASES[name])
    return orc.render(frame_camera("exponents, lean"), W, Hh, spp, np.zeros((spp, 2)))


@pytest.mark.parametrize("name", list(SOFT_CASES))
def test_soft_light_cases_on_oracle(name):
    """The cases are alive: a wide light leaves pixels with some of its samples occluded, the two sides of 0.9 draw different streams, and
    at scatter 0 every sample is the light's own direction - the frame of a directional light, whatever the count."""
    direction, samples, scatter = SOFT_CASES[name]
    frame, st = soft_oracle(name, 1)
    assert st["rays_traced"] == W * Hh * (1 + samples)                 # every pixel ray hits, the plane or the sphere
    if scatter == 0.0 or scatter == 2.0 ** -1074:
        orc = O.Oracle()
        soft_scene(orc, direction, samples, scatter, soft=False)
        hard, _ = orc.render(frame_camera("exponents, lean"), W, Hh, 1, np.zeros((1, 2)))
        assert np.array_equal(hard == 0.0, frame == 0.0) and np.allclose(frame, hard, rtol=1e-12, atol=0) and (frame > 0.0).any() and (direction[0] == 0.0 or (frame == 0.0).any())   # (straight down the shadow hides under the sphere)
    elif samples == 4 and scatter == _WIDE and direction[1] < -0.1:
        part = {round(float(v), 6) for v in (frame[:, :, 0] / np.maximum(frame[:, :, 0].max(), 1e-300)).ravel()}
        assert len(part) >= 6, f"{name}: no penumbra in {sorted(part)}"
    if name == "x^ = 0.9 + 2^-31":
        assert not np.array_equal(frame, soft_oracle("x^ = 0.9 - 2^-31", 1)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SOFT_CASES))
def test_soft_light_frames_on_device(hip, name):
    """Occluded sample counts are whole numbers: a count off by one moves a pixel by 1 / samples of the light, far outside the frame contract.
    The frames are the oracle's on the same streams, with its ray count, under every option."""
    soft_scene(hip, *SOFT_CASES[name])
    cam = frame_camera("exponents, lean")
    options = {"uniform_surface": (1, 0), "coherent_waves": (1, 0), "wave_samples": (1, 4, 16)}
    try:
        for spp in (1, 4):
            want, ost = soft_oracle(name, spp)
            base = None
            for values in itertools.product(*options.values()):
                for opt, v in zip(options, values):
                    hip.set_option(opt, v)
                got, st = hip.render(cam, W, Hh, spp, np.zeros((spp, 2)))
                if base is None:
                    base, st0 = got, st
                    assert np.array_equal(np.isnan(base), np.isnan(want)), f"{name}: NaN pixels differ from the oracle's"
                    H.assert_frames_match(np.nan_to_num(base), np.nan_to_num(want), what=f"{name}, {spp} samples")
                    assert np.array_equal(base == 0.0, want == 0.0) and st["rays_reference_equivalent"] == ost["rays_traced"]
                assert np.array_equal(bits(got), bits(base)) and all(st[k] == st0[k] for k in COUNTERS), f"{name}, {spp} samples: {dict(zip(options, values))} changes the frame or the counters"
    finally:
        hip.set_option("wave_samples", 0)
        for opt in ("uniform_surface", "coherent_waves"):
            hip.set_option(opt, 1)


# ---- soft lights: every sample direction replayed --------------------------------------------------------------------------------------

BORDER = 1e-9                                                       # no sample may pass closer to a decision than this (the issue's figure)


@functools.lru_cache(maxsize=None)
def soft_replay(name):
    """For the one-sample-per-pixel frame of a soft case: {(x, y): expected colour} over the pixels that look at the plane (all of them, or
    eight under 255 samples), from the occluded count of the pixel's own stream (seed, sample = pixel) - every direction restated in both
    arithmetics of tests/shading_tools.py - with the nearest any sample comes to a decision and to the rejection circle's rim."""
    direction, samples, scatter = SOFT_CASES[name]
    stored = S.stored_direction(direction)
    cam = frame_camera("exponents, lean")
    out, nearest, rims = {}, S.INF, []
    for y, x in itertools.product(range(Hh), range(W)):
        if samples == 255 and not (x % 4 == 1 and y % 4 == 1):
            continue
        o, d = O.ray_through_pixel(cam, W, Hh, x, y)
        if S.ball_margin(S.Binary64(), list(o), list(d)) is not None and S.ball_margin(S.Binary64(), list(o), list(d)) < 1e-3:
            continue                                                # the pixel looks at the ball, or grazes it
        t = -o[1] / d[1]
        origin = [o[0] + t * d[0], S.OFFSET, o[2] + t * d[2]]
        verdicts = []
        for A in (S.Exact, S.Binary64):
            K = A()
            dirs = S.soft_directions(K, stored, samples, scatter, ft.DEFAULT_SEED, y * W + x, rims=rims if A is S.Exact else None)
            got = [S.soft_occluded(K, [K.num(c) for c in origin], v) for v in dirs]
            verdicts.append([g[0] for g in got])
            if A is S.Exact:
                nearest = min([nearest] + [g[1] for g in got])
        assert verdicts[0] == verdicts[1], f"{name}, pixel ({x}, {y}): binary64 and exact arithmetic count differently"
        lit = (samples - sum(verdicts[0])) / samples                # Shading.fs:31
        out[(x, y)] = [lit * c * -stored[1] for c in S.D_COLOUR]     # the white plane's Lambert term under scaleColour intensity colour
    return out, nearest, min(rims)


def check_soft_counts(frame, name, who):
    want, _, _ = soft_replay(name)
    for (x, y), colour in want.items():
        assert all(abs(g - c) <= S.SUM_SLACK * abs(c) for g, c in zip(frame[y, x], colour)), f"{who}, {name}, pixel ({x}, {y}): {list(frame[y, x])}, by the replay {colour}"


@pytest.mark.parametrize("name", list(SOFT_CASES))
def test_soft_light_replay_and_oracle(name, capsys):
    want, nearest, rim = soft_replay(name)
    with capsys.disabled():
        print(f"\n  {name}: {len(want)} pixels replayed, nearest decision {nearest:.2e}, nearest rim {rim:.2e}", end="")
    assert len(want) >= 6 and nearest >= BORDER and rim >= 1e-12       # the counts are whole numbers both sides must hit
    check_soft_counts(soft_oracle(name, 1)[0], name, "oracle")
    direction, samples, scatter = SOFT_CASES[name]
    if samples == 4 and scatter == _WIDE and direction[1] < -0.1:
        assert len({tuple(c) for c in want.values()}) >= 3               # lit, part and dark pixels


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SOFT_CASES))
def test_soft_light_counts_on_device(hip, name):
    soft_scene(hip, *SOFT_CASES[name])
    frame, _ = hip.render(frame_camera("exponents, lean"), W, Hh, 1, np.zeros((1, 2)))
    check_soft_counts(frame, name, "device")


# ---- depth of field ----------------------------------------------------------------------------------------------------------------------

DOF_MAT = S.Material((0.8, 0.6, 0.4), 0.0, 0.0, 3.0)
DOF_LIGHTS = GENERIC_LIGHT + DOWN_LIGHT
DOF_SPP = 4
# name -> (focal length, aperture angle)
DOF_CASES = {"f 0, aperture 0": (0.0, 0.0), "f 2^-30, aperture 0": (2.0 ** -30, 0.0), "f 5, aperture 0": (5.0, 0.0), "f 1e8, aperture 0": (1e8, 0.0),
             "f 0, aperture 0.05": (0.0, 0.05), "f 2^-30, aperture 0.05": (2.0 ** -30, 0.05), "f 5, aperture 0.05": (5.0, 0.05), "f 1e8, aperture 1e-9": (1e8, 1e-9),
             "f 5, aperture pi/2": (5.0, math.pi / 2.0), "f 0, aperture pi/2": (0.0, math.pi / 2.0)}


def dof_camera(name):
    cam = frame_camera("exponents, lean")
    cam.has_focus, cam.focal_length, cam.aperture_angular_size = 1, DOF_CASES[name][0], DOF_CASES[name][1]
    return cam


@functools.lru_cache(maxsize=None)
def dof_rays(name):
    """Per pixel and sample: the pin-hole ray and the ray ImagePlane.depthOfFieldJitter makes of it, replayed in binary64 on the pixel's
    stream; the exact replay takes the same generator and gives the same direction to 1e-12."""
    f, aperture = DOF_CASES[name]
    cam = frame_camera("exponents, lean")
    pin_o, pin_d, o2, d2 = [], [], [], []
    for y, x in itertools.product(range(Hh), range(W)):
        o, d = O.ray_through_pixel(cam, W, Hh, x, y)
        for s in range(DOF_SPP):
            K, E = S.Binary64(), S.Exact()
            ro, rd = S.depth_of_field_ray(K, o, d, f, aperture, ft.DEFAULT_SEED, (y * W + x) * DOF_SPP + s)
            if s == 0:
                _, ed = S.depth_of_field_ray(E, o, d, f, aperture, ft.DEFAULT_SEED, (y * W + x) * DOF_SPP + s)
                assert K.branches == E.branches and all(abs(float(a) - b) <= 1e-12 for a, b in zip(ed, rd)), f"{name}, pixel ({x}, {y})"
            pin_o.append(o); pin_d.append(d); o2.append(ro); d2.append(rd)
    return np.array(pin_o), np.array(pin_d), np.array(o2), np.array(d2)


def check_dof(b, name, who):
    """The frame is the mean, in sample order, of colour_for_ray of the replayed rays; with aperture 0 the ray is the pin-hole ray along its
    own line: the pin-hole colour to the case's bound, and (focal length 0) the closest t scaled by |d|."""
    S.build_scene(b, [DOF_MAT], DOF_LIGHTS)
    frame, st = b.render(dof_camera(name), W, Hh, DOF_SPP, np.zeros((DOF_SPP, 2)))
    pin_o, pin_d, o2, d2 = dof_rays(name)
    shaded = b.colour_for_ray(o2, d2).reshape(Hh, W, DOF_SPP, 3)
    mean = (((shaded[:, :, 0] + shaded[:, :, 1]) + shaded[:, :, 2]) + shaded[:, :, 3]) / DOF_SPP
    H.assert_frames_match(frame, mean, what=f"{who}, {name}: the frame against its own samples' rays")
    f, aperture = DOF_CASES[name]
    if aperture == 0.0 and f <= 5.0:
        for k in range(0, W * Hh, 9):
            y, x = divmod(k, W)
            v = S.evaluate(S.Case(f"pixel ({x}, {y})", list(pin_o[k * DOF_SPP]), list(pin_d[k * DOF_SPP]), DOF_MAT, DOF_LIGHTS))
            assert S.error_ratio(frame[y, x], v) <= 1.0, f"{who}, {name}, pixel ({x}, {y}): {frame[y, x]}, the pin-hole colour {v.colour}"
        if f == 0.0:
            _, t_pin, _, _, _ = b.closest(pin_o, pin_d)
            _, t_dof, _, _, _ = b.closest(o2, d2)
            assert np.allclose(t_dof, t_pin * np.linalg.norm(pin_d, axis=1), rtol=1e-12, atol=0), f"{who}, {name}: closest t is not scaled by |d|"
    return frame, st


@pytest.mark.parametrize("name", list(DOF_CASES))
def test_depth_of_field_on_oracle(name):
    frame, _ = check_dof(O.Oracle(), name, "oracle")
    assert (frame > 0).any() or DOF_CASES[name][0] == 1e8              # (1e8 along a direction 0.4 % longer than its unit vector: the origin passes the plane)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DOF_CASES))
def test_depth_of_field_on_device(hip, name):
    want, ost = check_dof(O.Oracle(), name, "oracle")
    base, st0 = check_dof(hip, name, "device")
    H.assert_frames_match(base, want, what=f"{name}: against the oracle")
    assert np.array_equal(np.isnan(base), np.isnan(want)) and st0["rays_reference_equivalent"] == ost["rays_traced"]
    options = {"uniform_surface": (1, 0), "coherent_waves": (1, 0), "wave_samples": (1, 4, 16)}
    try:
        for values in itertools.product(*options.values()):
            for opt, v in zip(options, values):
                hip.set_option(opt, v)
            got, st = hip.render(dof_camera(name), W, Hh, DOF_SPP, np.zeros((DOF_SPP, 2)))
            assert np.array_equal(bits(got), bits(base)) and all(st[k] == st0[k] for k in COUNTERS), f"{name}: {dict(zip(options, values))} changes the frame or the counters"
    finally:
        hip.set_option("wave_samples", 0)
        for opt in ("uniform_surface", "coherent_waves"):
            hip.set_option(opt, 1)

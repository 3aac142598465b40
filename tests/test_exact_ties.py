"""Hit selection and CSG where hit distances tie exactly.

Family I: op(X, X') with X' built by the same calls as X - every hit of A ties with a hit of B on every ray, under any transform.
Family II: lattice rays o = P - k d through lattice targets of primitives under translations and per-axis scales by powers of two:
every product and sum up to the target hit is exact in binary64, so the device, the oracle and the rational reference of
tests/tie_tools.py must give the same bits, and rims, borders, apexes, tangent points and shared faces are met exactly.

The expectation on Family II is the rational reference.  The oracle is faithful to F#, whose cube side faces and solidCylinder bottom
cap carry cos 90 / sin 180 residues; on rays where an equality is decided inside one of those (residue rays) it is not consulted, on
every other kept ray it must equal the rational reference (a hard assertion of the CPU half).

Findings: none on the device; every Family II t came out bit-equal."""
import functools
import zlib

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from . import tie_tools as T
from .test_aov import _oracle_parity
from .test_far_from_origin import one_per_wave

F = T.F
N_RAYS = 160                                                       # per target class
OP_NAMES = list(T.OPS)
SINGLE_CASES = [(k, x) for k in T.SINGLES for x in T.TRANSFORMS]
PAIR_CASES = [(p, x) for p in T.PAIRS for x in ("bare", "scaled")]
OP2 = {"union": ft.SUBTRACT, "intersect": ft.UNION, "subtract": ft.EXCLUDE, "exclude": ft.INTERSECT}   # the inner operator of "nested"


def _seed(*parts):
    return zlib.crc32("/".join(parts).encode())


# =============================================================================================================================
# References, computed once per process and shared by the CPU and the GPU halves

class ClassRef:
    """One target class of a case: its rays (exact and as arrays) and, per scene tree, the verdict of every ray."""

    def __init__(self, points, ops, want, seed, opts=None):
        self.want = want
        opts = dict(opts or {})
        self.rays = T.lattice_rays(points, ops, opts.pop("n", N_RAYS), seed, tangent=want == "tangent", **opts)
        self.o, self.d, self.k = T.rays_as_arrays(self.rays)
        self.cache = T.LeafCache(self.rays)

    def verdicts(self, target):
        tree = T.scene_tree(target)
        return [T.judge(tree, self.cache, i) for i in range(len(self.rays))]


@functools.lru_cache(maxsize=None)
def single_reference(kind, xf):
    ops = T.TRANSFORMS[xf]
    target = T.prim(kind, ops, 0)
    out = {}
    for cls, (points, want) in T.single_classes(kind).items():
        ref = ClassRef(points, ops, want, _seed(kind, xf, cls))
        out[cls] = (ref, ref.verdicts(target))
    return target, out


@functools.lru_cache(maxsize=None)
def pair_reference(pair, xf):
    """(operand A, operand B, {class: ClassRef}, {(class, op, shape): verdicts}, {(op, shape): target tree})."""
    ops = T.TRANSFORMS[xf]
    (ka, oa), (kb, ob), classes = T.pair_case(pair)
    A, B = T.prim(ka, tuple(oa) + tuple(ops), 0), T.prim(kb, tuple(ob) + tuple(ops), 1)
    refs = {cls: ClassRef(spec[0], ops, spec[1], _seed(pair, xf, cls), *spec[2:]) for cls, spec in classes.items()}
    targets = {(op, shape): T.shaped(shape, T.OPS[op], A, B, OP2[op]) for op in OP_NAMES for shape in T.SHAPES}
    verdicts = {(cls, op, shape): refs[cls].verdicts(targets[(op, shape)]) for cls in refs for (op, shape) in targets}
    return A, B, refs, verdicts, targets


def expected_arrays(verdicts):
    """Of the kept rays: indices, hit flags, t, material colour and normal of the winner, whether t is an exact double, residue flags."""
    idx = np.array([i for i, v in enumerate(verdicts) if v.kept], dtype=np.int64)
    hit = np.array([verdicts[i].winner is not None for i in idx], dtype=np.int32)
    t, col, n, exact = np.zeros(idx.size), np.zeros((idx.size, 3)), np.zeros((idx.size, 3)), np.zeros(idx.size, dtype=bool)
    for j, i in enumerate(idx):
        w = verdicts[i].winner
        if w is not None:
            t[j], col[j], n[j], exact[j] = float(w.t), T.leaf_colour(w.leaf), w.n, T.is_small_dyadic(w.t)
    residue = np.array([verdicts[i].residue for i in idx], dtype=bool)
    return idx, hit, t, col, n, exact, residue


def assert_matches_exact(got, o, d, want, what):
    """hit flag and material colour equal; t bit for bit where the exact t is a double (every target hit is), else to helpers.TIGHT;
    normals to 1e-7 (the cone's apex: the zero vector; a NaN would have to meet a NaN); p = o + t d to helpers.TIGHT."""
    idx, hit, t, col, n, exact, _ = want
    ghit, gt, gp, gn, gc = (a[idx] for a in got)
    assert np.array_equal(ghit, hit), f"{what}: hit/miss differs on rays {idx[ghit != hit][:8]}"
    m = hit.astype(bool)
    assert np.array_equal(gc[m], col[m]), f"{what}: another leaf won on rays {idx[m][np.any(gc[m] != col[m], axis=1)][:8]}"
    e = m & exact
    assert np.array_equal(gt[e], t[e]), f"{what}: t not bit-equal on rays {idx[e][gt[e] != t[e]][:8]}: {gt[e][gt[e] != t[e]][:4]} vs {t[e][gt[e] != t[e]][:4]}"
    assert np.all(np.abs(gt[m] - t[m]) <= H.TIGHT * (1.0 + np.abs(t[m]))), f"{what}: t differs"
    nan = np.isnan(n)
    assert np.array_equal(np.isnan(gn[m]), nan[m]), f"{what}: NaN normals differ"
    diff = np.where(nan[m], 0.0, np.abs(gn[m] - n[m]))
    assert diff.size == 0 or diff.max() <= 1e-7, f"{what}: normals differ by {diff.max()} on rays {idx[m][np.any(diff > 1e-7, axis=1)][:8]}"
    p = o[idx] + t[:, None] * d[idx]
    assert np.all(np.abs(gp[m] - p[m]) <= H.TIGHT * (1.0 + np.abs(p[m]))), f"{what}: p differs"


def shadow_cases(verdicts, want):
    """For kept rays won on a flat face at an exactly representable t: (ray indices, max_dist == t, nextafter(t, inf)).  The first is
    not blocked (no hit has 0 <= t' < t: the winner is the closest), the second is - both decided by exact doubles."""
    idx, hit, t, _, _, exact, _ = want
    flat = np.array([hit[j] == 1 and exact[j] and (T.KIND_NAME[verdicts[i].winner.key[0]], verdicts[i].winner.sub) in T.FLAT
                     for j, i in enumerate(idx)], dtype=bool)
    return idx[flat], t[flat], np.nextafter(t[flat], np.inf)


def check_oracle_agrees(orc, ref, verdicts, what, must_agree_outside_residue=True):
    """Oracle all_hits against the exact sequence of every kept ray: count, order, t (bitwise where exact), normals (so flips), and
    its closest hit against the exact winner.  Returns the boolean mask (over all rays) of the kept rays on which the oracle equals
    the exact reference; outside the residue rays that must be every kept ray."""
    counts, t, _, n = orc.all_hits(ref.o, ref.d, cap=24)
    chit, ct, _, cn, ccol = orc.closest(ref.o, ref.d)
    agreed = np.zeros(len(verdicts), dtype=bool)
    for i, v in enumerate(verdicts):
        if not v.kept:
            continue
        assert all(h.leaf < 20 for h in v.hits), f"{what}: ray {i} hits a filler"
        ok = counts[i] == len(v.hits)
        for k, h in enumerate(v.hits if ok else []):
            tt = float(h.t)
            ok = ok and (t[i, k] == tt if T.is_small_dyadic(h.t) and not h.res else abs(t[i, k] - tt) <= 1e-12 * (1.0 + abs(tt)))
            ok = ok and (np.all(np.isnan(n[i, k])) if np.any(np.isnan(h.n)) else bool(np.max(np.abs(n[i, k] - h.n)) <= 1e-7))
        w = v.winner                                                 # and `closest` picks the same hit (a t of -1e-17 for 0 would not)
        ok = ok and bool(chit[i]) == (w is not None)
        if ok and w is not None:
            ok = abs(ct[i] - float(w.t)) <= 1e-12 * (1.0 + abs(float(w.t))) and tuple(ccol[i]) == T.leaf_colour(w.leaf) and bool(np.max(np.abs(cn[i] - w.n)) <= 1e-7)
        agreed[i] = ok
        if must_agree_outside_residue and not v.residue:
            assert ok, (f"{what}: ray {i} ({ref.rays[i]}) is no residue ray, yet the oracle gives {counts[i]} hits {t[i, :counts[i]]} / {n[i, :counts[i]]}, "
                        f"the exact reference {[(float(h.t), h.leaf, h.sub, h.flip) for h in v.hits]}")
    return agreed


def class_summary(ref, verdicts, agreed):
    kept = np.array([v.kept for v in verdicts])
    at_target = sum(1 for i, v in enumerate(verdicts) if v.kept and ref.k[i] >= 0 and any(h.t == ref.k[i] for h in v.hits))
    tied = sum(1 for v in verdicts if v.kept and v.tied)
    return {"kept": float(kept.mean()), "at_target": at_target, "tied": tied, "agreed": int(agreed.sum()), "kept_n": int(kept.sum())}


# =============================================================================================================================
# CPU half

def _h(t, leaf):
    return T.Hit(F(t), leaf, 0, False, np.array([0.0, 0.0, float(leaf + 1)]), False, None)


def test_csg_rules_on_hand_worked_ties():
    """Csg.fs by hand.  A0 = B0 < A1 = B1: the stable sort gives A0 B0 A1 B1, reached in the states (out, out), (in A, out), (in A, in B),
    (out, in B): OutsideIntoA, AIntoAB, ABleaveA, BIntoOutside."""
    a, b = [_h(2, 0), _h(5, 0)], [_h(2, 1), _h(5, 1)]
    types = []
    got = T.constructed_solid(ft.UNION, a, b, types=types)
    assert types == ["OutsideIntoA", "AIntoAB", "ABleaveA", "BIntoOutside"]
    seq = lambda hits: [(int(h.t), h.leaf, h.flip) for h in hits]
    assert seq(got) == [(2, 0, False), (5, 1, False)]                                            # Take, Discard, Discard, Take
    assert seq(T.constructed_solid(ft.INTERSECT, a, b)) == [(2, 1, False), (5, 0, False)]        # AIntoAB and ABleaveA
    assert seq(T.constructed_solid(ft.SUBTRACT, a, b)) == [(2, 0, False), (2, 1, True)]          # A's front, then B's front flipped
    assert seq(T.constructed_solid(ft.EXCLUDE, a, b)) == [(2, 0, False), (2, 1, True), (5, 0, True), (5, 1, False)]
    flipped = T.constructed_solid(ft.SUBTRACT, a, b)[1]
    assert np.array_equal(flipped.n, [0.0, 0.0, -2.0])
    for op in T.OPS.values():                                                                    # closest: the first of the near pair
        w = T.closest(T.constructed_solid(op, a, b))
        assert (int(w.t), w.leaf, w.flip) == ((2, 1, False) if op == ft.INTERSECT else (2, 0, False))
    # from inside (t0 < 0 < t1): union leaves through B's back, intersect through A's, subtract holds nothing, exclude A's back flipped
    a, b = [_h(-2, 0), _h(5, 0)], [_h(-2, 1), _h(5, 1)]
    res = {name: T.closest(T.constructed_solid(op, a, b)) for name, op in T.OPS.items()}
    assert res["subtract"] is None
    assert [(res[k].leaf, res[k].flip) for k in ("union", "intersect", "exclude")] == [(1, False), (0, False), (0, True)]
    # a far-root-first operand (Math.fs:10) sorts to the same sequence: the sort is by t, stable only among equals
    assert seq(T.constructed_solid(ft.EXCLUDE, [_h(5, 0), _h(2, 0)], [_h(5, 1), _h(2, 1)])) == [(2, 0, False), (2, 1, True), (5, 0, True), (5, 1, False)]
    # a touching pair A0 < A1 = B0 < B1 (the spheres at 4, 6, 6, 8): A1 is reached first, AIntoOutside, then B0 OutsideIntoB
    a, b = [_h(4, 0), _h(6, 0)], [_h(6, 1), _h(8, 1)]
    types = []
    assert seq(T.constructed_solid(ft.UNION, a, b, types=types)) == [(4, 0, False), (6, 0, False), (6, 1, False), (8, 1, False)]
    assert types == ["OutsideIntoA", "AIntoOutside", "OutsideIntoB", "BIntoOutside"]
    assert T.constructed_solid(ft.INTERSECT, a, b) == []                                         # touching solids share no volume
    assert seq(T.constructed_solid(ft.SUBTRACT, a, b)) == [(4, 0, False), (6, 0, False)]
    # the other way round (operand A is leaf 1 at 6, 8; B leaf 0 at 4, 6: B0 < B1 = A0 < A1): A0 comes first on the tie, while still inside B
    types = []
    assert seq(T.constructed_solid(ft.INTERSECT, b, a, types=types)) == [(6, 1, False), (6, 0, False)]   # a zero-width sliver: BIntoAB, ABleaveB
    assert types == ["OutsideIntoB", "BIntoAB", "ABleaveB", "AIntoOutside"]
    # a double root (a tangent ray, the cone's apex) A0 = A1 inside B: in and out of A at one t
    a, b = [_h(3, 0), _h(3, 0)], [_h(1, 1), _h(7, 1)]
    assert seq(T.constructed_solid(ft.INTERSECT, a, b)) == [(3, 0, False), (3, 0, False)]
    assert seq(T.constructed_solid(ft.SUBTRACT, a, b)) == []                                     # A never outside B, B's surfaces never inside A
    assert seq(T.constructed_solid(ft.SUBTRACT, b, a)) == [(1, 1, False), (3, 0, True), (3, 0, True), (7, 1, False)]
    # closest: negative t skipped, 0 kept, the first of equals wins; lightIsBlocked: t < max_dist strictly
    hits = [_h(-1, 0), _h(3, 1), _h(0, 2), _h(0, 3)]
    assert T.closest(hits).leaf == 2 and T.closest(hits[:1]) is None
    assert not T.light_is_blocked(hits[1:2], F(3)) and T.light_is_blocked(hits[1:2], F(3) + F(1, 2 ** 50)) and not T.light_is_blocked(hits[:1], F(9))


def test_exact_primitives_on_hand_worked_rays():
    """The model-frame primitives at their boundaries, by hand."""
    C = T.Cmps()
    one, half = F(1), F(1, 2)
    # cylinder rim (closed): from (3, 1, 0) along (-1, 0, 0) the roots are 4 (far, first) and 2, both at py = 1
    assert [(h[0], h[1]) for h in T.cylinder((F(3), one, F(0)), (F(-1), F(0), F(0)), C)] == [(4, 0), (2, 1)]
    assert T.cylinder((F(3), one + F(1, 2 ** 20), F(0)), (F(-1), F(0), F(0)), C) == []
    # circle rim (open): straight down onto (1, 0, 0) misses, a hair inside hits
    assert T.circle((one, F(2), F(0)), (F(0), F(-1), F(0)), C) == []
    assert [h[0] for h in T.circle((one - F(1, 2 ** 20), F(2), F(0)), (F(0), F(-1), F(0)), C)] == [2]
    # square corner (closed)
    assert [h[0] for h in T.square((one, F(2), one), (F(0), F(-1), F(0)), C)] == [2]
    # the cone's apex (0, 1, 0): c = 0 and b^2 = 4 a c + ... gives discriminant 0 for any ray through it: a double root at t = 3
    hits = T.cone((F(-3), F(-2), F(-6)), (one, one, F(2)), C)
    assert [h[0] for h in hits] == [3, 3] and all(h[2] == (0.0, 0.0, 0.0) for h in hits)
    # a < 0 (steeper than the side): the near root comes first.  Down the axis offset by 1/2: the side is met at y = 1/2 (t = 3/2), and
    # the mirror nappe above the apex at y = 3/2 (t = 1/2) is filtered out
    assert [(h[0], h[1]) for h in T.cone((half, F(2), F(0)), (F(0), F(-1), F(0)), C)] == [(F(3, 2), 1)]
    # tangent to the sphere at (1, 0, 0): t0 == t1
    assert [h[0] for h in T.sphere((one, F(-2), F(0)), (F(0), one, F(0)), C)] == [2, 2]
    # cube, through the corner (1/2, 1/2, 1/2) along (-1, -1, -1): top, right and back at t = 1, then bottom, left, front at t = 2,
    # in the order bottom, top, left, right, front, back
    hits = T.cube((F(3, 2),) * 3, (F(-1),) * 3, C)
    assert [(h[0], h[1]) for h in hits] == [(2, 0), (1, 1), (2, 2), (1, 3), (2, 4), (1, 5)]
    # solidCylinder down the axis: top, bottom, and no sides (a = 0 is degenerate: dropped from the exact family)
    with pytest.raises(T.Irrational):
        T.solid_cylinder((F(0), F(3), F(0)), (F(0), F(-1), F(0)), C)
    # from (-3, 5/2, 0) along (1, -1/2, 0): the top cap at t = 3 (x = 0); the side's far root 4 (y = 1/2) first, its near root 2 is at
    # y = 3/2 and filtered; the bottom plane is met at x = 2, outside
    assert [(h[0], h[1]) for h in T.solid_cylinder((F(-3), F(5, 2), F(0)), (one, F(-1, 2), F(0)), C)] == [(3, 0), (4, 2)]
    # the keeping rule: an equality of exact doubles is kept, one of thirds is not, a margin of 1e-12 is not
    assert T.robust([(F(1), F(1), True, (), False)]) and not T.robust([(F(1, 3), F(1, 3), True, (), False)])
    assert not T.robust([(F(1), F(1) + F(1, 10 ** 12), True, (), False)]) and T.robust([(F(1), F(1) + F(1, 10 ** 8), True, (), False)])
    assert not T.robust([(F(0), F(0), False, (), False)]) and not T.robust([(F(1), F(1), True, (F(1, 3),), False)])


@functools.lru_cache(maxsize=None)
def _host():
    return ft.Context(host_only=True)


def _want_at_target(ref, v, i):
    """What the exact reference must say at the target of ray i (k >= 0 or behind)."""
    k = F(int(ref.k[i]))
    n_at = sum(h.t == k for h in v.hits)
    return {"hit": n_at >= 1, "miss": n_at == 0, "double": n_at == 2, "tangent": n_at == 2, None: True}[ref.want]


@pytest.mark.parametrize("kind,xf", SINGLE_CASES)
def test_family2_single_primitives_exact_vs_oracle(kind, xf, capsys):
    target, classes = single_reference(kind, xf)
    orc = O.Oracle()
    T.build_scene(orc, target)
    ctx = _host()
    T.build_scene(ctx, target)
    info = ctx.scene_info()
    assert info["items"] == 3 and info["leaves"] == 3
    for cls, (ref, verdicts) in classes.items():
        what = f"{kind} {xf} {cls}"
        for i, v in enumerate(verdicts):
            if v.kept:
                assert _want_at_target(ref, v, i), f"{what}: ray {i} {ref.rays[i]}: {[(h.t, h.sub) for h in v.hits]}"
                assert np.all(ref.d[i] != 0.0) or ref.want == "tangent"
        agreed = check_oracle_agrees(orc, ref, verdicts, what)
        s = class_summary(ref, verdicts, agreed)
        with capsys.disabled():
            print(f"\n  {what}: kept {s['kept']:.0%}, {s['at_target']} hits with t == k, {s['tied']} tied winners, oracle agrees on {s['agreed']} of {s['kept_n']}", end="")
        assert s["kept"] >= 0.60, what
        hit, t, _, _, col = orc.closest(ref.o, ref.d)
        n_oracle_at_k = int(np.sum((hit == 1) & (t == ref.k) & agreed))
        if ref.want == "miss":
            counts, ts, _, _ = orc.all_hits(ref.o, ref.d, cap=8)
            assert not any(ts[i, j] == ref.k[i] for i in np.nonzero(agreed)[0] for j in range(counts[i])), f"{what}: the open rim is hit"
        elif not (kind == "cube" and cls in ("edge", "corner")) and cls != "rim_bottom":
            assert n_oracle_at_k >= 32, f"{what}: only {n_oracle_at_k} oracle winners at t == k"
        if ref.want in ("double", "tangent"):
            assert s["tied"] >= 32


@pytest.mark.parametrize("pair,xf", PAIR_CASES)
def test_family2_pairs_exact_vs_oracle(pair, xf, capsys):
    A, B, refs, verdicts, targets = pair_reference(pair, xf)
    orc, ctx = O.Oracle(), _host()
    words = {}
    for (op, shape), target in targets.items():
        facts = T.tree_facts(target)
        assert (facts["marks"], facts["marks_under_pair"]) == T.expected_facts(shape), (op, shape, facts)
        T.build_scene(ctx, target)
        info = ctx.scene_info()
        n_leaves = {"fold": 2, "merge": 2}.get(shape, 3) + 2
        assert info["items"] == 3 and info["leaves"] == n_leaves, (op, shape, info)
        words[(op, shape)] = info["program_words"]
        T.build_scene(orc, target)
        for cls, ref in refs.items():
            v = verdicts[(cls, op, shape)]
            agreed = check_oracle_agrees(orc, ref, v, f"{pair} {xf} {op} {shape} {cls}")
            s = class_summary(ref, v, agreed)
            assert s["kept"] >= 0.60, (pair, xf, op, shape, cls, s)
            if shape == "fold":
                with capsys.disabled():
                    print(f"\n  {pair} {xf} {op} {cls}: kept {s['kept']:.0%}, {s['at_target']} hits with t == k, {s['tied']} tied winners, "
                          f"oracle agrees on {s['agreed']} of {s['kept_n']}", end="")
    for op in OP_NAMES:
        # the fused pair is three words in front of the generic sequence; a one-child group adds no word of its own
        assert words[(op, "fold")] - words[(op, "merge")] == 3, words
        for shape in T.SHAPES:
            tied = sum(v.kept and v.tied for cls in refs for v in verdicts[(cls, op, shape)])
            at_k = {cls: sum(1 for i, v in enumerate(verdicts[(cls, op, shape)]) if v.kept and v.winner is not None and v.winner.t == refs[cls].k[i]) for cls in refs}
            assert tied >= 64, (pair, xf, op, shape, tied)
            assert sum(at_k.values()) >= 32, (pair, xf, op, shape, at_k)


SHADOW_CASES = [("single", k, x) for k in ("plane", "square", "circle", "cube", "solidCylinder") for x in ("bare", "scaled")] + [("pair", "capped", "bare"), ("pair", "capped", "scaled")]


def _shadow_scenes(which, name, xf):
    """(target, ClassRef, verdicts) of every scene of a case that the shadow bounds are checked on."""
    if which == "single":
        target, classes = single_reference(name, xf)
        return [(target, ref, v) for ref, v in classes.values()]
    _, _, refs, verdicts, targets = pair_reference(name, xf)
    return [(targets[(op, "fold")], ref, verdicts[(cls, op, "fold")]) for op in OP_NAMES for cls, ref in refs.items()]


@pytest.mark.parametrize("which,name,xf", SHADOW_CASES)
def test_shadow_bounds_at_flat_faces(which, name, xf, capsys):
    """max_dist == t: not blocked (t < max_dist is strict); the next double above t: blocked.  On the exact reference for every winner on
    a flat face, and on the oracle where its t is the exact one: not from a rotated face (those are an ulp off: `max_dist == t` is then
    decided by the residue), on rays where it agrees with the exact reference."""
    orc = O.Oracle()
    n_exact = n_oracle = 0
    for target, ref, v in _shadow_scenes(which, name, xf):
        T.build_scene(orc, target)
        idx, at, above = shadow_cases(v, expected_arrays(v))
        agreed = check_oracle_agrees(orc, ref, v, "shadow bounds", must_agree_outside_residue=False)
        for i, md0, md1 in zip(idx, at, above):
            assert not T.light_is_blocked(v[i].hits, F(md0)) and T.light_is_blocked(v[i].hits, F(md1))
        keep = agreed[idx] & np.array([not v[i].residue and not v[i].winner.res for i in idx], dtype=bool)
        assert not orc.blocked(ref.o[idx][keep], ref.d[idx][keep], at[keep]).any()
        assert orc.blocked(ref.o[idx][keep], ref.d[idx][keep], above[keep]).all()
        n_exact, n_oracle = n_exact + idx.size, n_oracle + int(keep.sum())
    with capsys.disabled():
        print(f"\n  shadow bounds {name} {xf}: {n_exact} rays on the exact reference, {n_oracle} of them on the oracle", end="")
    assert n_oracle >= 32


# ---- Family I ------------------------------------------------------------------------------------------------------------------------

def family1_target(kind, op, shape):
    A, B = T.identical_operands(kind)
    return T.shaped(shape, T.OPS[op], A, B, OP2[op])


@pytest.mark.parametrize("kind", list(H.PRIMS))
def test_family1_identical_operands_on_the_oracle(kind, capsys):
    """op(X, X'): every hit of A ties with B's.  The closed forms (from the rules, test_csg_rules_on_hand_worked_ties): with X's own hits
    t0 <= t1 (or the one hit t0), union is [A0, B1] ([A0]), intersect [B0, A1] ([B0]), subtract [A0, B0 flipped], exclude [A0, B0
    flipped, A1 flipped, B1] ([A0, B0 flipped]); and in every shape the oracle's sequence is Csg.fs applied to the operands' own."""
    orc, ctx, single = O.Oracle(), _host(), O.Oracle()
    o, d = T.family1_rays(kind)
    leaves = T.OracleLeaves(single, o, d)
    A, B = T.identical_operands(kind)
    for op in OP_NAMES:
        for shape in T.SHAPES:
            target = family1_target(kind, op, shape)
            assert (T.tree_facts(target)["marks"], T.tree_facts(target)["marks_under_pair"]) == T.expected_facts(shape)
            T.build_scene(ctx, target)
            assert ctx.scene_info()["items"] == 3
            T.build_scene(orc, target)
            counts, t, _, n = orc.all_hits(o, d, cap=16)
            hit, ct, _, cn, col = orc.closest(o, d)
            tied = 0
            for i in range(o.shape[0]):
                want = T.evaluate(T.scene_tree(target), _no_fillers(leaves.at(i)))
                assert counts[i] == len(want), (kind, op, shape, i)
                for k, h in enumerate(want):
                    assert t[i, k] == h.t and (np.array_equal(n[i, k], h.n) or np.all(np.isnan(h.n))), (kind, op, shape, i, k)
                w = T.closest(want)
                assert (w is not None) == bool(hit[i])
                if w is not None:
                    assert ct[i] == w.t and tuple(col[i]) == T.leaf_colour(w.leaf), (kind, op, shape, i)
                    tied += 1                                      # every hit of X is a tie with X'
                if shape == "fold":
                    a, b = leaves.at(i)(A), leaves.at(i)(B)
                    assert [h.t for h in a] == [h.t for h in b] or kind == "plane"      # (the plane is hit where the square is missed)
                    s = sorted(a, key=lambda h: h.t)
                    if len(s) in (1, 2) and len(a) == len(b):
                        last = len(s) - 1
                        closed = {"union": [(0, 0, 0)] if last == 0 else [(0, 0, 0), (last, 1, 0)],
                                  "intersect": [(0, 1, 0)] if last == 0 else [(0, 1, 0), (last, 0, 0)],
                                  "subtract": [(0, 0, 0), (0, 1, 1)],
                                  "exclude": [(0, 0, 0), (0, 1, 1)] if last == 0 else [(0, 0, 0), (0, 1, 1), (last, 0, 1), (last, 1, 0)]}[op]
                        assert [(0 if h.t == s[0].t else last, h.leaf, int(h.flip)) for h in want] == closed, (kind, op, i)
            if shape == "fold":
                with capsys.disabled():
                    print(f"\n  identical {kind} {op}: {tied} of {o.shape[0]} rays won by a tied hit", end="")
            assert tied >= 64, (kind, op, shape, tied)


def _no_fillers(leaf):
    """The fillers are far from every Family I ray (asserted by the hit counts): their leaves give no hits."""
    def fn(p):
        return [] if p[3] >= 20 else leaf(p)
    fn.C = None
    return fn


# =============================================================================================================================
# GPU half

def _both_layouts(hip, o, d, centre, seed, limit=4096):
    """hip.closest for the rays packed 64 to a wave, and for each ray alone in a wave of certain misses; <= `limit` rays per call."""
    packed = hip.closest(o, d)
    alone = [np.zeros(o.shape[0], dtype=np.int32), np.zeros(o.shape[0]), np.zeros((o.shape[0], 3)), np.zeros((o.shape[0], 3)), np.zeros((o.shape[0], 3))]
    step = limit // 64
    for s in range(0, o.shape[0], step):
        oo, dd = one_per_wave(o[s:s + step], d[s:s + step], centre, seed + s)
        got = hip.closest(oo, dd)
        for a, g in zip(alone, got):
            a[s:s + step] = g[::64]
            assert not got[0].reshape(-1, 64)[:, 1:].any()
    return packed, tuple(alone)


def _blocked_both_layouts(hip, o, d, md, centre, seed, limit=4096):
    packed = hip.blocked(o, d, md)
    alone = np.zeros(o.shape[0], dtype=np.int32)
    step = limit // 64
    for s in range(0, o.shape[0], step):
        oo, dd = one_per_wave(o[s:s + step], d[s:s + step], centre, seed + s)
        mm = np.repeat(md[s:s + step], 64)
        alone[s:s + step] = hip.blocked(oo, dd, mm)[::64]
    return packed, alone


def _centre(ops):
    return np.array([float(c) for c in T.to_world((0, 0, 0), ops)])


def _check_family2_on_device(hip, orc, target, ref, verdicts, ops, what):
    want = expected_arrays(verdicts)
    idx = want[0]
    if idx.size == 0:
        return
    o, d = ref.o, ref.d
    for layout, got in zip(("packed", "one per wave"), _both_layouts(hip, o, d, _centre(ops), 11)):
        assert_matches_exact(got, o, d, want, f"{what}, {layout}")
    # the oracle, on the kept rays where it equals the exact reference
    agreed = check_oracle_agrees(orc, ref, verdicts, what, must_agree_outside_residue=False)
    if agreed.any():
        H.assert_hits_match(tuple(a[agreed] for a in hip.closest(o, d)), _nan_to_zero(orc.closest(o[agreed], d[agreed])), what=what + " against the oracle")
    # shadows: max_dist == t and the next double, for winners on flat faces
    sidx, at, above = shadow_cases(verdicts, want)
    if sidx.size:
        for md, blocked in ((at, 0), (above, 1)):
            for layout, got in zip(("packed", "one per wave"), _blocked_both_layouts(hip, o[sidx], d[sidx], md, _centre(ops), 13)):
                assert np.all(got == blocked), f"{what}, {layout}: max_dist {'above' if blocked else 'at'} t: rays {sidx[got != blocked][:8]}"


def _nan_to_zero(hits):
    return tuple(np.where(np.isnan(a), 0.0, a) if a.dtype == np.float64 else a for a in hits)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,xf", SINGLE_CASES)
def test_family2_single_primitives_on_device(hip, kind, xf):
    target, classes = single_reference(kind, xf)
    orc = O.Oracle()
    T.build_scene(orc, target)
    T.build_scene(hip, target)
    assert hip.scene_info()["items"] == 3
    for cls, (ref, verdicts) in classes.items():
        _check_family2_on_device(hip, orc, target, ref, verdicts, T.TRANSFORMS[xf], f"{kind} {xf} {cls}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("pair,xf", PAIR_CASES)
def test_family2_pairs_on_device(hip, pair, xf, shape):
    A, B, refs, verdicts, targets = pair_reference(pair, xf)
    orc = O.Oracle()
    for op in OP_NAMES:
        target = targets[(op, shape)]
        T.build_scene(orc, target)
        T.build_scene(hip, target)
        assert hip.scene_info()["items"] == 3
        for cls, ref in refs.items():
            _check_family2_on_device(hip, orc, target, ref, verdicts[(cls, op, shape)], T.TRANSFORMS[xf], f"{pair} {xf} {op} {shape} {cls}")


def _assert_nan_aware(got, want, what):
    ghit, gt, gp, gn, gc = got
    whit, wt, wp, wn, wc = want
    assert np.array_equal(np.isnan(gn), np.isnan(wn)), f"{what}: NaN normals differ"
    H.assert_hits_match((ghit, gt, gp, np.nan_to_num(gn), gc), (whit, wt, wp, np.nan_to_num(wn), wc), what=what)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("kind", list(H.PRIMS))
def test_family1_rays_on_device(hip, kind, shape):
    """closest, lightIsBlocked and getColourForRay (shadow rays from, and one reflection off, a tied surface) against the oracle."""
    orc = O.Oracle()
    o, d = T.family1_rays(kind)
    centre = np.array([0.3, 0.3, -0.1])
    md = np.abs(np.random.default_rng(3).normal(size=o.shape[0])) * 4.0 / np.linalg.norm(d, axis=1)
    for op in OP_NAMES:
        what = f"identical {kind} {op} {shape}"
        target = family1_target(kind, op, shape)
        for b in (orc, hip):
            _build_reflective(b, target)
        want = orc.closest(o, d)
        packed, alone = _both_layouts(hip, o[:512], d[:512], centre, 17)
        _assert_nan_aware(hip.closest(o, d), want, what)
        _assert_nan_aware(alone, tuple(a[:512] for a in want), what + ", one per wave")
        wb = orc.blocked(o, d, md)
        assert np.array_equal(hip.blocked(o, d, md), wb), f"{what}: lightIsBlocked differs"
        assert np.array_equal(_blocked_both_layouts(hip, o[:512], d[:512], md[:512], centre, 19)[1], wb[:512]), f"{what}: lightIsBlocked differs, one per wave"
        got, ref = hip.colour_for_ray(o, d, max_depth=2), orc.colour_for_ray(o, d, max_depth=2)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN colours differ"
        H.assert_frames_match(np.where(nan, 0.0, got)[:, None, :], np.where(nan, 0.0, ref)[:, None, :], what=what)


def _build_reflective(b, target):
    """build_scene with the operands' materials reflective, so that getColourForRay spawns a reflection off the tied surface."""
    b.clear()

    def node(t):
        if t[0] == "prim":
            n = b.primitive(t[1])
            if t[2]:
                n = b.transform(list(T.float_ops(t[2])), n)
            return b.material(n, colour=T.leaf_colour(t[3]), reflectance=0.4, shineyness=5.0)
        if t[0] == "group":
            return b.group([node(c) for c in t[1]])
        return b.csg(t[1], node(t[2]), node(t[3]))
    b.set_objects(b.group([node(t) for t in [target] + T.FILLERS]))
    b.add_directional((0.3, -1.0, 0.5), (1, 1, 1))
    b.add_positional((1.0, 6.0, -2.0), (1.0, 0.01, 0.02), (0.6, 0.6, 0.6))
    b.commit()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(H.PRIMS))
def test_family1_frames_on_device(hip, kind):
    """The coherent route (bundle cull, then the pair), which explicit rays do not take: small frames as shipped and with
    coherent_waves = 0 against the oracle, and render_aov's hit, n and material colour at every pixel."""
    orc = O.Oracle()
    cam = ft.make_camera((2.5, 2.0, -4.5), (0.3, 0.3, -0.1), (0, 1, 0), H.deg(35.0), 72 / 56)
    try:
        for k, op in enumerate(OP_NAMES):
            shape = T.SHAPES[k % len(T.SHAPES)] if kind != "sphere" else "fold"
            target = family1_target(kind, op, shape)
            for b in (orc, hip):
                _build_reflective(b, target)
            for spp in (2, 4):
                jit = ft.jitter_pattern(spp)
                want, ost = orc.render(cam, 72, 56, spp, jit, seed=ft.DEFAULT_SEED)
                nan = np.isnan(want)
                for coherent in (1, 0):
                    hip.set_option("coherent_waves", coherent)
                    got, st = hip.render(cam, 72, 56, spp, jit, seed=ft.DEFAULT_SEED)
                    what = f"identical {kind} {op} {shape}, {spp} samples, coherent_waves {coherent}"
                    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pixels differ"
                    assert H.assert_frames_match(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what=what) < 1e-6
                    assert st["rays_reference_equivalent"] == ost["rays_traced"]
            hip.set_option("coherent_waves", 1)
            aov = _oracle_parity(hip, orc, cam, 72, 56, None, f"identical {kind} {op} {shape}: render_aov")
            assert (aov["leaf"] >= 0).sum() >= 40 or kind in ("square", "plane", "circle")
    finally:
        hip.set_option("coherent_waves", 1)

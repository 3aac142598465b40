"""Dual-quaternion skinning (ft_sg_set_mesh_bones_dq / ft_debug_skin_dq): the skin of test_skinning.py posed by a palette of
unit dual quaternions, the vertices made by k_skin_dq into the buffer the refit reads (ft_skin.hip) and scanned there by the morph kernels.

The promise under test: set_mesh_bones_dq(node, P) followed by any commit gives every bit that set_mesh_triangles(node, V) gives on a twin
node without a skin, V = functracer_amd.skin_blend_dq(shape, index, weight, P) - the formula of the header in numpy, one elementwise IEEE
operation per step.  Every comparison against the twin is bitwise.  The one place with a tolerance is the geometry test, which holds the
twin itself against a 60-digit evaluation of the unrounded formula, to a running error bound that the test derives operation by
operation."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi

from . import bvh_tools as B
from . import helpers as H
from .test_light_space_shadows import light_space
from .test_mesh_refit import CAT, RES, SPP, Recorder, _ground_scene, answers, assert_same_answers, assert_same_topology, contexts, same  # noqa: F401 (contexts: a fixture)
from .test_morph_targets import replay_scan, same_trees, targets_of, view_of
from .test_skinning import LABELS, _fma, _moved_scene, _options, _small, palette, skin_of

MESHES = dict(CAT)
for _n in (85, 86):                                                  # 255 and 258 corners: one short of a block of 256, two past it
    MESHES[f"blob({_n})"] = B._entry(f"blob({_n})", B.blob(_n))


def rigid(n_bones, seed, centre=(0.0, 0.0, 0.0), radius=1.0, amount=1.0):
    """n_bones rigid motions from a seeded generator: unit quaternions [n, 4] of a rotation about an arbitrary axis, about `centre`, and
    translations [n, 3] of a fraction of `radius` more."""
    rng = np.random.default_rng(seed)
    centre = np.asarray(centre, dtype=np.float64)
    r, t = np.zeros((n_bones, 4)), np.zeros((n_bones, 3))
    for b in range(n_bones):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = amount * rng.uniform(-0.6, 0.6)
        K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        R = np.eye(3) + math.sin(ang) * K + (1.0 - math.cos(ang)) * (K @ K)
        r[b] = [math.cos(0.5 * ang), *(math.sin(0.5 * ang) * axis)]
        t[b] = centre - R @ centre + amount * rng.uniform(-0.2, 0.2, size=3) * radius
    return r, t


def dq_palette(n_bones, seed, centre=(0.0, 0.0, 0.0), radius=1.0, amount=1.0, negate=True):
    """[n_bones, 8] dual quaternions of rigid(); negate: the odd bones are stored as -D (the same motions), so that the sign select has work."""
    out = ft.dual_quaternions(*rigid(n_bones, seed, centre, radius, amount))
    if negate:
        out[1::2] *= -1.0
    return out


def pose_of(e, J, n_bones, label, seed=3, amount=1.0, negate=True):
    base = e.tris.reshape(-1, 9)
    index, weight = skin_of(base.shape[0], J, n_bones, label, seed)
    return base, index, weight, dq_palette(n_bones, seed + 100, e.centre, e.radius, amount, negate)


def skin_bytes(base, J, n_bones, rest=True, per_bone=64):
    corners = base.shape[0] * 3
    return (base.size * 8 if rest else 0) + corners * 4 + corners * J * 8 + n_bones * per_bone


def counts(ctx, node):
    s = ctx.skin_dq(node)
    return s["device_commits"], s["device_meshes"], s["host_meshes"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_bindings_declare_the_dq_calls():
    hdr = open(os.path.join(H.ROOT, "include", "functracer_hip.h")).read()
    assert "#define FT_ABI_VERSION 2" in hdr and "#define FT_MAX_SKIN_BONES 256" in hdr
    assert re.search(r"int32_t ft_sg_set_mesh_bones_dq\(ft_context\* ctx, ft_node mesh, const double\* dual_quaternions, int32_t n_bones\);", hdr)
    assert re.search(r"int32_t ft_debug_skin_dq\(ft_context\* ctx, ft_node mesh, int64_t counts\[4\]\);", hdr)
    for said in ("V_i = (p_i + 2*h_i) + 2*m_i", "a NaN g does not negate", "Scale and shear cannot be expressed", "non-finite coordinate", "stays welded"):
        assert said in hdr, said
    lib = C.CDLL(ft.HIP_LIB)
    doc = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    for name in ("ft_sg_set_mesh_bones_dq", "ft_debug_skin_dq"):
        assert hasattr(lib, name), name
        assert re.search(r"\[<DllImport\(Lib\)>\] extern int " + name + r"\(", doc), name
        assert name in [s[0] for s in _capi.SKIN_DQ_SIGNATURES]
    for name in ("set_mesh_bones_dq", "skin_dq"):
        assert callable(getattr(ft.Context, name)), name
    assert callable(ft.skin_blend_dq) and callable(ft.dual_quaternions)
    d = ft.dual_quaternions([[1.0, 0, 0, 0], [0.0, 0, 1.0, 0]], [[2.0, 4.0, 6.0], [1.0, 0.0, 0.0]])
    assert np.array_equal(d, [[1, 0, 0, 0, 0, 1, 2, 3], [0, 0, 1, 0, 0, 0, 0, 0.5]])   # 0.5 * (0, t) (x) r: i j = k


def test_the_setter_refuses_bad_arguments_and_changes_nothing():
    ctx = ft.Context(host_only=True)
    hd = _small(ctx)
    lib = ft.hip_lib()
    T0, info0 = ctx.mesh_trees(), ctx.scene_info()
    e = CAT["blob(9)"]
    _, index, weight, dq = pose_of(e, 2, 3, "mixed")
    pd = _capi.dptr(dq)
    set_dq = lambda *a: lib.ft_sg_set_mesh_bones_dq(*a)             # noqa: E731
    kind = lambda: ctx.skin_dq(hd["flat"])["palette_kind"]          # noqa: E731
    assert set_dq(ctx._ctx, hd["flat"], pd, 3) == -1                # a palette without a skin
    assert "no skin" in ctx.last_error()
    ctx.set_mesh_skin(hd["flat"], index, weight)
    assert set_dq(None, hd["flat"], pd, 3) == -1 and set_dq(ctx._ctx, hd["xf"], pd, 3) == -1    # a null context, a transform node
    assert set_dq(ctx._ctx, -1, pd, 3) == -1 and set_dq(ctx._ctx, 10_000, pd, 3) == -1
    assert set_dq(ctx._ctx, hd["flat"], None, 3) == -1
    big = np.ascontiguousarray(np.resize(dq, (257, 8)))
    for n in (-1, 257):
        assert set_dq(ctx._ctx, hd["flat"], _capi.dptr(big), n) == -1, n
    for n in (1, 2):                                                 # the skin uses bone 2
        assert set_dq(ctx._ctx, hd["flat"], pd, n) == -1, n
    for bad in (np.nan, np.inf, -np.inf):
        for at in (3, 7):                                            # the real part, the dual part
            db = dq.copy()
            db[1, at] = bad
            assert set_dq(ctx._ctx, hd["flat"], _capi.dptr(db), 3) == -1, (bad, at)
    cnt = (C.c_int64 * 4)()
    assert lib.ft_debug_skin_dq(ctx._ctx, hd["xf"], cnt) == -1 and lib.ft_debug_skin_dq(None, hd["flat"], cnt) == -1 and lib.ft_debug_skin_dq(ctx._ctx, hd["flat"], None) == -1
    assert lib.ft_debug_skin_dq(ctx._ctx, -1, cnt) == -1
    assert kind() == 0
    ctx.commit_deformed()                                            # nothing was marked: the commit of before, bit for bit
    same_trees(ctx.mesh_trees(), T0, "after the refused calls")
    ctx.commit()
    same_trees(ctx.mesh_trees(), T0, "after the refused calls and a full commit")
    assert ctx.scene_info() == info0
    bones = palette(3, 5)                                            # and a refused call leaves a palette of either kind in force as it is
    ctx.set_mesh_bones(hd["flat"], bones)
    assert set_dq(ctx._ctx, hd["flat"], pd, 2) == -1 and kind() == 1
    ctx.commit_deformed()
    T1 = ctx.mesh_trees()
    ctx.set_mesh_bones_dq(hd["flat"], dq)
    ctx.commit_deformed()
    T2 = ctx.mesh_trees()
    db = dq.copy()
    db[2, 0] = np.nan
    assert set_dq(ctx._ctx, hd["flat"], _capi.dptr(db), 3) == -1 and lib.ft_sg_set_mesh_bones(ctx._ctx, hd["flat"], _capi.dptr(bones), 2) == -1 and kind() == 2
    ctx.commit()
    same_trees(ctx.mesh_trees(), T2, "a refused call under a dual-quaternion palette")
    ctx.set_mesh_bones(hd["flat"], bones)
    ctx.commit()
    same_trees(ctx.mesh_trees(), T1, "the matrix palette again")
    ctx.close()


def test_the_order_rules_of_the_two_palette_kinds():
    e = CAT["blob(65)"]
    base, index, weight, dq = pose_of(e, 4, 6, "mixed")
    bones = palette(6, 103, e.centre, e.radius)
    ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)

    def expect(tris, kind, what):
        _moved_scene(fresh, tris, 0.0)
        same_trees(ctx.mesh_trees(), fresh.mesh_trees(), what)
        assert ctx.skin_dq(m)["palette_kind"] == kind, what
    m, _ = _moved_scene(ctx, base, 0.0)
    ctx.set_mesh_skin(m, index, weight)
    ctx.commit_deformed()
    expect(base, 0, "a skin alone")
    ctx.set_mesh_bones(m, bones)
    ctx.commit_deformed()
    expect(ft.skin_blend(base, index, weight, bones), 1, "matrices")
    ctx.set_mesh_bones_dq(m, dq)                                     # replaces the matrices
    ctx.commit_deformed()
    expect(ft.skin_blend_dq(base, index, weight, dq), 2, "dual quaternions replace matrices")
    assert counts(ctx, m) == (0, 0, 1) and ctx.skin(m)["host_meshes"] == 0, "each debug call counts its own kind"
    ctx.set_mesh_bones(m, bones)                                     # and back
    ctx.commit_deformed()
    expect(ft.skin_blend(base, index, weight, bones), 1, "matrices replace dual quaternions")
    assert counts(ctx, m) == (0, 0, 0) and ctx.skin(m)["host_meshes"] == 1
    ctx.set_mesh_bones(m, np.zeros((0, 12)))
    ctx.commit_deformed()
    expect(base, 0, "none")
    ctx.set_mesh_bones_dq(m, dq)
    ctx.commit()                                                     # a full commit skins on demand
    expect(ft.skin_blend_dq(base, index, weight, dq), 2, "dual quaternions, full commit")
    ctx.set_mesh_bones(m, np.zeros((0, 12)))                         # n_bones = 0 through the matrix call removes a dual-quaternion palette
    ctx.commit_deformed()
    expect(base, 0, "n_bones = 0 through ft_sg_set_mesh_bones")
    ctx.set_mesh_bones(m, bones)
    ctx.set_mesh_bones_dq(m, np.zeros((0, 8)))                       # and the other way round
    ctx.commit_deformed()
    expect(base, 0, "n_bones = 0 through ft_sg_set_mesh_bones_dq")
    ctx.set_mesh_bones_dq(m, dq)
    ctx.commit_deformed()
    shape2 = base + 0.125
    ctx.set_mesh_triangles(m, shape2)                                # a new U under the palette in force
    ctx.commit_deformed()
    expect(ft.skin_blend_dq(shape2, index, weight, dq), 2, "set_mesh_triangles under a dual-quaternion palette re-poses the new shape")
    targets, w = targets_of(e, 2), [0.3, -0.2]
    ctx.set_mesh_targets(m, targets)                                 # the base is U, not V
    ctx.set_mesh_weights(m, w)
    ctx.commit_deformed()
    blended = ft.morph_blend(shape2, targets, w)
    expect(ft.skin_blend_dq(blended, index, weight, dq), 2, "blend the shape, then skin it")
    ctx.commit_deformed()                                            # nothing marked
    assert counts(ctx, m) == (0, 0, 0)
    ctx.set_mesh_skin(m, index[:, :, :2], weight[:, :, :2])          # a new skin removes the palette and marks the node
    ctx.commit_deformed()
    expect(blended, 0, "set_mesh_skin removes a dual-quaternion palette")
    ctx.close(), fresh.close()


# ---- the formula, exactly ----------------------------------------------------------------------------------------------------------
def _sqrt_rounded(x):
    """The double nearest to sqrt(x), x a Fraction >= 0 that is a double: the candidate math.sqrt gives is accepted when the exact
    radicand lies between the squares of the two half-way points to its neighbours."""
    if x == 0:
        return 0.0
    n = math.sqrt(float(x))
    lo, hi = (Fraction(n) + Fraction(math.nextafter(n, 0.0))) / 2, (Fraction(n) + Fraction(math.nextafter(n, math.inf))) / 2
    assert lo * lo <= x <= hi * hi, "math.sqrt is not correctly rounded here"
    return n


def _formula(shape, index, weight, dq, fused=False, sign_rule=True):
    """The header's formula in exact rational arithmetic, rounded to double after every step.  fused: every multiply-add is one rounding
    (math.fma) - what the library must NOT compute.  sign_rule False: without the antipodality test."""
    F = Fraction
    rnd = lambda q: F(float(q))                                      # noqa: E731
    mul = lambda a, b: rnd(a * b)                                    # noqa: E731
    add = lambda a, b: rnd(a + b)                                    # noqa: E731
    sub = lambda a, b: rnd(a - b)                                    # noqa: E731

    def mad(a, b, c):                                                # a * b + c
        return F(_fma(float(a), float(b), float(c))) if fused else add(mul(a, b), c)

    def msub(a, b, c, d):                                            # a * b - c * d
        return F(_fma(float(a), float(b), -float(mul(c, d)))) if fused else sub(mul(a, b), mul(c, d))

    def cross(a, b):
        return [msub(a[(i + 1) % 3], b[(i + 2) % 3], a[(i + 2) % 3], b[(i + 1) % 3]) for i in range(3)]
    p_all = shape.reshape(-1, 3)
    idx, w_all = index.reshape(p_all.shape[0], -1), weight.reshape(p_all.shape[0], -1)
    out = np.zeros_like(p_all)
    for c in range(p_all.shape[0]):
        p = [F(float(v)) for v in p_all[c]]
        R0 = [F(float(v)) for v in dq[idx[c, 0], :4]]
        a = None
        for j in range(idx.shape[1]):
            D = [F(float(v)) for v in dq[idx[c, j]]]
            ws = F(float(w_all[c, j]))
            if j > 0 and sign_rule:
                g = mad(D[3], R0[3], mad(D[2], R0[2], mad(D[1], R0[1], mul(D[0], R0[0]))))
                ws = -ws if g < 0 else ws
            a = [mul(ws, D[k]) for k in range(8)] if j == 0 else [mad(ws, D[k], a[k]) for k in range(8)]
        n2 = mad(a[3], a[3], mad(a[2], a[2], mad(a[1], a[1], mul(a[0], a[0]))))
        n = F(_sqrt_rounded(n2))
        if n == 0:                                                   # s = inf; the real part 0 * inf = NaN reaches every coordinate
            out[c] = np.nan
            continue
        s = rnd(1 / n)
        u = [mul(a[k], s) for k in range(8)]
        w, v, e, f = u[0], u[1:4], u[4], u[5:8]
        vp = cross(v, p)
        cc = [mad(w, p[i], vp[i]) for i in range(3)]
        h = cross(v, cc)
        vf = cross(v, f)
        for i in range(3):
            m = add(msub(w, f[i], e, v[i]), vf[i])
            out[c, i] = float(mad(2, m, mad(2, h[i], p[i])))          # (doubling is exact: fusing it changes nothing)
    return out.reshape(-1, 9)


def _exact_inputs(label, J=4):
    e = CAT["blob(9)"]
    base = np.concatenate([e.tris.reshape(-1, 9), e.tris.reshape(-1, 9) + 1e3])[:17]   # 51 corners, near and far from the origin
    index, weight = skin_of(17, J, 6, label)
    return base, index, weight, dq_palette(6, 103, e.centre, e.radius)   # bones 1, 3 and 5 negated


@pytest.mark.parametrize("label", LABELS)
def test_skin_blend_dq_is_the_formula_rounded_once_per_step(label):
    base, index, weight, dq = _exact_inputs(label)
    got = ft.skin_blend_dq(base, index, weight, dq)
    assert got.shape == (17, 9) and np.isfinite(got).all(), label
    assert np.array_equal(got, _formula(base, index, weight, dq)), label
    for j in (1, 2, 3):                                              # fewer influences: the first j slots
        fewer = ft.skin_blend_dq(base, index[:, :, :j], weight[:, :, :j], dq)   # ("cancel" cut to three slots blends some corners to zero: NaN on both sides)
        assert np.array_equal(fewer, _formula(base, index[:, :, :j], weight[:, :, :j], dq), equal_nan=True), (label, j)
        assert np.isfinite(fewer).all() or (label, j) == ("cancel", 3), (label, j)


def test_a_fused_step_would_change_the_chosen_inputs():
    base, index, weight, dq = _exact_inputs("mixed")
    assert (_formula(base, index, weight, dq, fused=True) != ft.skin_blend_dq(base, index, weight, dq)).any(), "the never-fused case is vacuous: fusing changes no bit of it"
    assert (_formula(base, index[:, :, :1], weight[:, :, :1], dq, fused=True) != ft.skin_blend_dq(base, index[:, :, :1], weight[:, :, :1], dq)).any(), "J = 1: fusing changes no bit"


def test_negated_bones_give_the_bits_of_the_palette_without_the_negation():
    e = CAT["blob(65)"]
    base = e.tris.reshape(-1, 9)
    for J, label in ((2, "equal"), (4, "mixed"), (3, "equal")):
        index, weight = skin_of(base.shape[0], J, 8, label)
        index[:, :, 0] &= ~1                                         # slot 0 names an even bone: not one of the negated ones
        plain = dq_palette(8, 9, e.centre, e.radius, negate=False)
        negated = dq_palette(8, 9, e.centre, e.radius, negate=True)
        assert same(negated[0::2], plain[0::2]) and same(negated[1::2], -plain[1::2])
        assert (index[:, :, 1:] & 1).any(), "no negated bone is used"
        v = ft.skin_blend_dq(base, index, weight, plain)
        assert same(ft.skin_blend_dq(base, index, weight, negated), v), (J, label)
        # and the rule is what does it: without the antipodality test the negated palette gives other vertices
        assert (_formula(base[:6], index[:6], weight[:6], negated, sign_rule=False) != v[:6]).any(), (J, label)
        assert np.array_equal(_formula(base[:6], index[:6], weight[:6], negated), v[:6]), (J, label)
        ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)   # the library's host twin agrees
        m, _ = _moved_scene(ctx, base, 0.0)
        ctx.set_mesh_skin(m, index, weight)
        ctx.set_mesh_bones_dq(m, negated)
        ctx.commit_deformed()
        _moved_scene(fresh, v, 0.0)
        same_trees(ctx.mesh_trees(), fresh.mesh_trees(), f"negated bones, J = {J}, {label}")
        ctx.close(), fresh.close()


# ---- the geometry, against 60 digits ------------------------------------------------------------------------------------------------
EPS = mpmath.mpf(2) ** -53                                           # the relative error of one IEEE double operation (round to nearest)
TINY = mpmath.mpf(2) ** -1075                                        # and its absolute error where the result is subnormal


class Run:
    """A value of the unrounded formula at 60 digits and a bound on how far the double evaluation can be from it - a running error
    analysis: an operation's result differs from the exact result of the exact operands by what the operands' errors propagate to
    (first the exact rule of the operation, with the error products kept) plus one rounding, EPS times the largest magnitude the computed
    result can have.  Nothing is taken from the code under test: the bound follows from the operations of the formula alone."""

    def __init__(self, v, err=0):
        self.v, self.err = mpmath.mpf(v), mpmath.mpf(err)

    @staticmethod
    def _rounded(v, prop):
        return Run(v, prop + EPS * (abs(v) + prop) + TINY)

    def __mul__(self, o):
        return Run._rounded(self.v * o.v, abs(self.v) * o.err + abs(o.v) * self.err + self.err * o.err)

    def __add__(self, o):
        return Run._rounded(self.v + o.v, self.err + o.err)

    def __sub__(self, o):
        return Run._rounded(self.v - o.v, self.err + o.err)

    def __neg__(self):
        return Run(-self.v, self.err)

    def twice(self):
        return Run(2 * self.v, 2 * self.err)                         # exact

    def sqrt(self):
        assert self.v > self.err
        return Run._rounded(mpmath.sqrt(self.v), mpmath.sqrt(self.v) - mpmath.sqrt(self.v - self.err))

    def reciprocal(self):
        assert self.v > self.err
        return Run._rounded(1 / self.v, 1 / (self.v - self.err) - 1 / self.v)


def _running(shape, index, weight, dq):
    """(V, bound): the unrounded formula per corner at 60 digits, and the running error bound of its double evaluation."""
    def cross(a, b):
        return [a[(i + 1) % 3] * b[(i + 2) % 3] - a[(i + 2) % 3] * b[(i + 1) % 3] for i in range(3)]
    p_all = shape.reshape(-1, 3)
    idx, w_all = index.reshape(p_all.shape[0], -1), weight.reshape(p_all.shape[0], -1)
    V, bound = [], []
    with mpmath.workdps(60):
        for c in range(p_all.shape[0]):
            p = [Run(float(x)) for x in p_all[c]]
            R0 = [Run(float(x)) for x in dq[idx[c, 0], :4]]
            a = None
            for j in range(idx.shape[1]):
                D = [Run(float(x)) for x in dq[idx[c, j]]]
                ws = Run(float(w_all[c, j]))
                if j > 0:
                    g = ((D[0] * R0[0] + D[1] * R0[1]) + D[2] * R0[2]) + D[3] * R0[3]
                    assert abs(g.v) > g.err, "the sign of g is decided by rounding: not a case for this test"
                    ws = -ws if g.v < 0 else ws
                q = [ws * D[k] for k in range(8)]
                a = q if j == 0 else [a[k] + q[k] for k in range(8)]
            n = (((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + a[3] * a[3]).sqrt()
            s = n.reciprocal()
            u = [a[k] * s for k in range(8)]
            w, v, e, f = u[0], u[1:4], u[4], u[5:8]
            vp = cross(v, p)
            cc = [vp[i] + w * p[i] for i in range(3)]
            h, vf = cross(v, cc), cross(v, f)
            out = [(p[i] + h[i].twice()) + ((w * f[i] - e * v[i]) + vf[i]).twice() for i in range(3)]
            V.append([o.v for o in out])
            bound.append([o.err for o in out])
    return V, bound


def _motion(d):
    """The rigid motion a dual quaternion (8 doubles) stands for, at 60 digits: the rotation matrix of its normalised real part and the
    translation 2 * (w f - e v + v x f) of the normalised whole."""
    n = mpmath.sqrt(sum(mpmath.mpf(float(x)) ** 2 for x in d[:4]))
    w, x, y, z, e, f0, f1, f2 = (mpmath.mpf(float(k)) / n for k in d)
    R = mpmath.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    t = mpmath.matrix([2 * (w * f0 - e * x + (y * f2 - z * f1)), 2 * (w * f1 - e * y + (z * f0 - x * f2)), 2 * (w * f2 - e * z + (x * f1 - y * f0))])
    return R, t


def _worst(got, V, bound):
    return max(float(abs(mpmath.mpf(float(g)) - x) / b) for grow, xrow, brow in zip(got.reshape(-1, 3), V, bound) for g, x, b in zip(grow, xrow, brow))


def test_one_hot_weights_give_the_bones_rigid_motion():
    e = CAT["blob(9)"]
    r, t = rigid(5, 31, e.centre, e.radius)
    dq = ft.dual_quaternions(r, t)
    dq[1::2] *= -1.0
    base = e.tris.reshape(-1, 9)
    index, weight = skin_of(base.shape[0], 3, 5, "one-hot")
    got = ft.skin_blend_dq(base, index, weight, dq)
    V, bound = _running(base, index, weight, dq)
    worst = _worst(got, V, bound)
    print(f"\n  one-hot: largest error / running bound {worst:.3g}, largest bound {float(max(max(b) for b in bound)):.3g}", end="")
    assert worst <= 1.0
    with mpmath.workdps(60):
        for b in range(5):                                           # what the palette holds is the motion it was made from, and a rigid one
            R, tt = _motion(dq[b])
            assert mpmath.norm(R * R.T - mpmath.eye(3)) < mpmath.mpf(10) ** -50 and abs(mpmath.det(R) - 1) < mpmath.mpf(10) ** -50
            assert all(abs(tt[i] - float(t[b, i])) <= 8 * float(EPS) * (1.0 + np.abs(t[b]).max()) for i in range(3)), b
        p_all = base.reshape(-1, 3)
        for c in range(p_all.shape[0]):                              # the unrounded formula is R p + t of slot 0's bone, whatever bones the zero weights name
            R, tt = _motion(dq[index.reshape(-1, 3)[c, 0]])
            want = R * mpmath.matrix([mpmath.mpf(float(x)) for x in p_all[c]]) + tt
            for i in range(3):
                assert abs(V[c][i] - want[i]) < mpmath.mpf(10) ** -45, (c, i)
                assert abs(mpmath.mpf(float(got.reshape(-1, 3)[c, i])) - want[i]) <= bound[c][i] + mpmath.mpf(10) ** -45, (c, i)


def test_a_twist_keeps_its_distance_from_the_axis_where_the_linear_blend_collapses():
    ang = 0.999 * math.pi                                            # bone 1 is bone 0 turned by this about y
    rng = np.random.default_rng(4)
    y = rng.uniform(-1.0, 1.0, size=(8, 3))
    phi = rng.uniform(0.0, 2.0 * math.pi, size=(8, 3))
    rest = math.hypot(1.0, 0.5)                                      # 1.118033988749895
    base = np.stack([rest * np.cos(phi), y, rest * np.sin(phi)], axis=-1).reshape(-1, 9)
    base[0, :3] = [1.0, 0.25, 0.5]
    index = np.broadcast_to(np.array([0, 1], dtype=np.int32), (8, 3, 2)).copy()
    weight = np.full((8, 3, 2), 0.5)
    dq = ft.dual_quaternions([[1.0, 0, 0, 0], [math.cos(0.5 * ang), 0, math.sin(0.5 * ang), 0]], np.zeros((2, 3)))
    got = ft.skin_blend_dq(base, index, weight, dq)
    V, bound = _running(base, index, weight, dq)
    worst = _worst(got, V, bound)
    assert worst <= 1.0
    p, q = base.reshape(-1, 3), got.reshape(-1, 3)
    ratio = 0.0
    with mpmath.workdps(60):
        for c in range(p.shape[0]):
            d0 = mpmath.sqrt(mpmath.mpf(float(p[c, 0])) ** 2 + mpmath.mpf(float(p[c, 2])) ** 2)
            d1 = mpmath.sqrt(mpmath.mpf(float(q[c, 0])) ** 2 + mpmath.mpf(float(q[c, 2])) ** 2)
            exact = mpmath.sqrt(V[c][0] ** 2 + V[c][2] ** 2)
            assert abs(exact - d0) < mpmath.mpf(10) ** -45            # the unrounded blend is a rotation about y
            allowed = mpmath.sqrt(bound[c][0] ** 2 + bound[c][2] ** 2)   # | |a| - |b| | <= |a - b|
            assert abs(d1 - d0) <= allowed + mpmath.mpf(10) ** -45, (c, float(d1), float(d0))
            assert abs(mpmath.mpf(float(q[c, 1])) - float(p[c, 1])) <= bound[c][1], c
            ratio = max(ratio, float(abs(d1 - d0) / allowed))
    print(f"\n  twist: largest error / running bound {worst:.3g}, distance from the axis: largest change / bound {ratio:.3g}, "
          f"largest bound {float(max(max(b) for b in bound)):.3g}", end="")
    assert f"{math.hypot(q[0, 0], q[0, 2]):.15f}" == "1.118033988749895"   # (1, y, 0.5): its distance in the rest pose, to every printed digit
    # why the feature exists: the matrices of the same two motions, blended linearly, lose more than 99 % of that distance
    R = np.array([[math.cos(ang), 0.0, math.sin(ang), 0.0], [0.0, 1.0, 0.0, 0.0], [-math.sin(ang), 0.0, math.cos(ang), 0.0]])
    bones = np.stack([np.eye(3, 4), R]).reshape(2, 12)
    lin = ft.skin_blend(base, index, weight, bones).reshape(-1, 3)
    assert (np.hypot(lin[:, 0], lin[:, 2]) < 0.01 * np.hypot(p[:, 0], p[:, 2])).all()


# ---- host-only contexts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 4])
@pytest.mark.parametrize("name", ["blob(9)", "degenerate", "identical"])
def test_host_only_dq_bones_give_the_bits_of_explicit_vertices(name, J):
    e = CAT[name]
    ctx, twin, fresh = ft.Context(host_only=True), ft.Context(host_only=True), ft.Context(host_only=True)
    for label in LABELS:
        if (label == "cancel" and J != 4) or (label == "tiny" and J == 1):
            continue
        base, index, weight, dq = pose_of(e, J, 7, label)
        v = ft.skin_blend_dq(base, index, weight, dq)
        assert np.isfinite(v).all()
        for commit in ("commit", "commit_moved", "commit_deformed"):
            what = f"{name}, J = {J}, {label}, {commit}"
            (m, xf), (m2, xf2) = _moved_scene(ctx, base, 0.0), _moved_scene(twin, base, 0.0)
            ctx.set_mesh_skin(m, index, weight)
            ctx.set_mesh_bones_dq(m, dq)
            twin.set_mesh_triangles(m2, v)
            shift = 0.0
            if commit == "commit_moved":                             # with a pose pending: the full commit
                shift = 1.5
                ctx.set_transform(xf, [("translate", (shift, 0, 0))])
                twin.set_transform(xf2, [("translate", (shift, 0, 0))])
            getattr(ctx, commit)()
            getattr(twin, commit)()
            _moved_scene(fresh, v, shift)
            got = ctx.mesh_trees()
            same_trees(got, twin.mesh_trees(), what + " (set_mesh_triangles)")
            same_trees(got, fresh.mesh_trees(), what + " (fresh graph)")
            assert all(same(x, y) for x, y in zip(ctx.leaf_matrices(), fresh.leaf_matrices())), what
            if commit == "commit_deformed":
                s, mo = ctx.skin_dq(m), ctx.morph(m)
                assert (s["device_commits"], s["device_meshes"], s["host_meshes"], s["palette_kind"]) == (0, 0, 1, 2), what
                assert ctx.skin(m)["resident_bytes"] == 0 and ctx.skin(m)["host_meshes"] == 0, what
                assert not mo["from_device"] and same(mo["scan"][:7], replay_scan(v)), what
    for c in (ctx, twin, fresh):
        c.close()


def test_a_mesh_welded_in_its_rest_pose_stays_welded():
    rng = np.random.default_rng(12)
    points = rng.normal(size=(40, 3))
    pidx, pw = rng.integers(0, 9, size=(40, 4)).astype(np.int32), rng.uniform(-0.5, 1.0, size=(40, 4))
    faces = rng.integers(0, 40, size=(120, 3))                       # every point is the corner of several triangles
    base, index, weight = points[faces].reshape(-1, 9), pidx[faces], pw[faces]
    dq = dq_palette(9, 8)
    v = ft.skin_blend_dq(base, index, weight, dq).reshape(-1, 3)
    assert np.isfinite(v).all()
    flat = faces.reshape(-1)
    for p in range(40):
        rows = v[flat == p]
        assert len(rows) and all(same(r, rows[0]) for r in rows), p
    ctx, fresh = ft.Context(host_only=True), ft.Context(host_only=True)
    m, _ = _moved_scene(ctx, base, 0.0)
    ctx.set_mesh_skin(m, index, weight)
    ctx.set_mesh_bones_dq(m, dq)
    ctx.commit_deformed()
    _moved_scene(fresh, v.reshape(-1, 9), 0.0)
    same_trees(ctx.mesh_trees(), fresh.mesh_trees(), "welded")
    ctx.close(), fresh.close()


def _zero_blend(n_tris):
    """Weights (0.5, -0.5) on one bone: the blend is zero, s = inf and every vertex NaN."""
    index = np.ones((n_tris, 3, 2), dtype=np.int32)
    weight = np.broadcast_to(np.array([0.5, -0.5]), (n_tris, 3, 2)).copy()
    return index, weight


def test_a_zero_blend_is_refused_and_the_old_commit_stays():
    ctx = ft.Context(host_only=True)
    e = CAT["blob(9)"]
    base, index, weight, dq = pose_of(e, 2, 3, "equal")
    zi, zw = _zero_blend(base.shape[0])
    assert np.isnan(ft.skin_blend_dq(base, zi, zw, dq)).all()
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    T0 = ctx.mesh_trees()
    ctx.set_mesh_skin(rec.meshes[0], zi, zw)
    ctx.set_mesh_bones_dq(rec.meshes[0], dq)
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    same_trees(ctx.mesh_trees(), T0, "after the refused commit")
    fresh = ft.Context(host_only=True)                               # (a host-only context renders nothing: the old commit is looked at as it lies; the GPU test renders it)
    B.build_scene(fresh, base)
    same_trees(ctx.mesh_trees(), fresh.mesh_trees(), "the old commit")
    assert ctx.scene_info() == fresh.scene_info()
    ctx.set_mesh_skin(rec.meshes[0], index, weight)
    ctx.set_mesh_bones_dq(rec.meshes[0], dq)
    ctx.commit_deformed()
    B.build_scene(fresh, ft.skin_blend_dq(base, index, weight, dq))
    same_trees(ctx.mesh_trees(), fresh.mesh_trees(), "the pose after the refusal")
    ctx.close(), fresh.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
# each mesh with each builder; J = 1 .. 4, 1 / 3 / 256 bones and the five weight sets spread over them; the odd bones of every palette negated
CASES = [(0, "blob(7)", 1, 3, "one-hot"), (0, "blob(65)", 2, 256, "equal"), (0, "blob(257)", 4, 3, "cancel"), (0, "blob(85)", 3, 256, "mixed"),
         (0, "blob(86)", 4, 3, "tiny"), (0, "degenerate", 2, 1, "tiny"), (0, "flat", 1, 256, "mixed"), (0, "identical", 4, 1, "equal"),
         (3, "blob(7)", 4, 256, "cancel"), (3, "blob(65)", 1, 1, "one-hot"), (3, "blob(257)", 2, 3, "tiny"), (3, "blob(85)", 4, 3, "equal"),
         (3, "blob(86)", 3, 256, "mixed"), (3, "degenerate", 4, 3, "equal"), (3, "flat", 2, 1, "one-hot"), (3, "identical", 3, 3, "mixed")]


def test_the_gpu_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == {0, 3} and {c[2] for c in CASES} == {1, 2, 3, 4} and {c[3] for c in CASES} == {1, 3, 256} and {c[4] for c in CASES} == set(LABELS)
    assert MESHES["blob(85)"].tris.shape[0] * 3 == 255 and MESHES["blob(86)"].tris.shape[0] * 3 == 258
    for builder, name, J, n_bones, label in CASES:
        base, index, weight, dq = pose_of(MESHES[name], J, n_bones, label)
        assert np.isfinite(ft.skin_blend_dq(base, index, weight, dq)).all(), (name, label)
        if n_bones > 1 and J > 1:                                    # the select takes both sides among the first 64 corners: within one wave
            i64 = index.reshape(-1, J)[:64]
            flips = (i64[:, 1:] & 1) != (i64[:, :1] & 1)
            assert flips.any() and not flips.all(), (name, label)


@pytest.mark.gpu
@pytest.mark.parametrize("builder,name,J,n_bones,label", CASES)
def test_dq_bones_give_every_bit_that_explicit_vertices_give(contexts, builder, name, J, n_bones, label):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, bvh_builder=builder)
    e = MESHES[name]
    what = f"builder {builder}, {name}, J = {J}, {n_bones} bones, {label}"
    base, index, weight, dq = pose_of(e, J, n_bones, label)
    v = ft.skin_blend_dq(base, index, weight, dq)
    view = view_of(v)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    node = rec.meshes[0]
    T0 = ctx.mesh_trees()
    commits, lin = ctx.skin_dq(node)["device_commits"], ctx.skin(node)["device_commits"]
    ctx.set_mesh_skin(node, index, weight)
    ctx.set_mesh_bones_dq(node, dq)
    ctx.commit_deformed()
    s, m = ctx.skin(node), ctx.morph(node)
    assert counts(ctx, node) == (commits + 1, 1, 0) and ctx.skin_dq(node)["palette_kind"] == 2, what
    assert (s["device_commits"], s["device_meshes"], s["host_meshes"]) == (lin, 0, 0), what + ": ft_debug_skin counted a dual-quaternion skin"
    assert s["resident_bytes"] == skin_bytes(base, J, n_bones), what
    assert (m["device_meshes"], m["host_meshes"], m["from_device"]) == (0, 0, True), what
    assert m["scan"][7] == 1.0 and same(m["scan"][:7], replay_scan(v)), f"{what}: the device scan is not scan_mesh's"
    got, T1 = answers(ctx, view, v.reshape(-1, 3, 3)), ctx.mesh_trees()
    if label != "cancel":
        assert got["hit"].any() and (got["frame"] != got["frame"][0, 0]).any(), f"{what}: the mesh is not in the view"
    assert_same_topology(T0, T1, what)
    twin.set_mesh_triangles(rec2.meshes[0], v)                       # the twin node without a skin
    twin.commit_deformed()
    assert_same_answers(got, answers(twin, view, v.reshape(-1, 3, 3)), what + " (twin)")
    same_trees(T1, twin.mesh_trees(), what + " (twin)")
    ctx.set_option("skin_on_device", 0)                              # the host route: the same bits
    ctx.set_mesh_bones_dq(node, dq)
    ctx.commit_deformed()
    m = ctx.morph(node)
    assert counts(ctx, node) == (commits + 1, 0, 1) and not m["from_device"], what
    assert same(m["scan"][:7], replay_scan(v)), what
    same_trees(ctx.mesh_trees(), T1, what + " (skin_on_device 0)")
    assert same(ctx.render(B.camera(*view), RES, RES, SPP, ft.jitter_pattern(SPP))[0], got["frame"]), what + " (skin_on_device 0)"
    ctx.set_option("skin_on_device", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["bone-255-everywhere", "bone-255-and-0", "one-bone-of-many"])
def test_the_last_bone_of_a_full_palette_and_one_bone_for_every_corner(contexts, case):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin)
    e = CAT["blob(257)"]
    base, index, weight, dq = pose_of(e, 2, 256, "equal")
    if case == "bone-255-everywhere":
        index[:] = 255
    elif case == "bone-255-and-0":
        index[:, :, 0], index[:, :, 1] = 255, 0                      # (bone 255 is stored negated, bone 0 is not)
    else:
        index[:] = 17                                                # every lane reads the same bone
    v = ft.skin_blend_dq(base, index, weight, dq)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    ctx.set_mesh_skin(rec.meshes[0], index, weight)
    ctx.set_mesh_bones_dq(rec.meshes[0], dq)
    ctx.commit_deformed()
    assert counts(ctx, rec.meshes[0])[1:] == (1, 0) and same(ctx.morph(rec.meshes[0])["scan"][:7], replay_scan(v))
    twin.set_mesh_triangles(rec2.meshes[0], v)
    twin.commit_deformed()
    same_trees(ctx.mesh_trees(), twin.mesh_trees(), case)
    cam, jit = B.camera(*view_of(v)), ft.jitter_pattern(SPP)
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0]), case


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["device", "morph_on_device 0", "skin_on_device 0"])
def test_morph_then_dq_skin_in_one_commit(contexts, route):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, morph_on_device=0 if route == "morph_on_device 0" else 1, skin_on_device=0 if route == "skin_on_device 0" else 1)
    e = CAT["blob(257)"]
    base, index, weight, _ = pose_of(e, 4, 12, "mixed")
    targets = targets_of(e, 3)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    node = rec.meshes[0]
    ctx.set_mesh_targets(node, targets)
    ctx.set_mesh_skin(node, index, weight)
    for w, seed in (([0.3, -0.2, 0.5], 1), ([0.1, 0.6, 0.0], 2)):
        pal = dq_palette(12, 200 + seed, e.centre, e.radius)
        v = ft.skin_blend_dq(ft.morph_blend(base, targets, w), index, weight, pal)
        ctx.set_mesh_weights(node, w)
        ctx.set_mesh_bones_dq(node, pal)
        ctx.commit_deformed()
        s, m = ctx.skin_dq(node), ctx.morph(node)
        if route == "device":
            assert (s["device_meshes"], s["host_meshes"], m["device_meshes"], m["host_meshes"], m["from_device"]) == (1, 0, 1, 0, True)
            assert ctx.skin(node)["resident_bytes"] == skin_bytes(base, 4, 12, rest=False), "the shape comes from the blend: no rest shape is resident"
        else:                                                        # the host route by rule: V is made by GraphNode::vertices
            assert (s["device_meshes"], s["host_meshes"], m["device_meshes"], m["host_meshes"], m["from_device"]) == (0, 1, 0, 1, False)
        assert same(m["scan"][:7], replay_scan(v)), route
        twin.set_mesh_triangles(rec2.meshes[0], v)
        twin.commit_deformed()
        same_trees(ctx.mesh_trees(), twin.mesh_trees(), route)
        cam, jit = B.camera(*view_of(v)), ft.jitter_pattern(SPP)
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0]), route
    _options(ctx, twin)


@pytest.mark.gpu
def test_all_kinds_of_mesh_in_one_commit(contexts):
    ctx, twin = contexts("work"), contexts("twin")
    _options(ctx, twin)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_multi(rec)
    B.build_multi(rec2)
    node = {part[0]: h for part, h in zip(B.MULTI_PARTS, rec.meshes)}
    cam, jit = B.camera(*B.MULTI_VIEW), ft.jitter_pattern(SPP)
    T0 = ctx.mesh_trees()
    new = {}
    e = CAT["blob(257)"]                                             # dual quaternions
    base, index, weight, dq = pose_of(e, 3, 20, "mixed")
    ctx.set_mesh_skin(node["blob(257)"], index, weight)
    ctx.set_mesh_bones_dq(node["blob(257)"], dq)
    new["blob(257)"] = ft.skin_blend_dq(base, index, weight, dq)
    e7 = CAT["blob(7)"]                                              # matrices
    b7 = e7.tris.reshape(-1, 9)
    i7, w7 = skin_of(b7.shape[0], 2, 4, "equal")
    bones = palette(4, 17, e7.centre, e7.radius, amount=0.3)
    ctx.set_mesh_skin(node["blob(7)"], i7, w7)
    ctx.set_mesh_bones(node["blob(7)"], bones)
    new["blob(7)"] = ft.skin_blend(b7, i7, w7, bones)
    mb, targets, w = CAT["blob(1025)"].tris.reshape(-1, 9), targets_of(CAT["blob(1025)"], 2), [0.3, 0.05]   # morph targets
    ctx.set_mesh_targets(node["blob(1025)"], targets)
    ctx.set_mesh_weights(node["blob(1025)"], w)
    new["blob(1025)"] = ft.morph_blend(mb, targets, w)
    new["blob(8)"] = CAT["blob(8)"].tris.reshape(-1, 9) * 1.01        # explicit vertices
    ctx.set_mesh_triangles(node["blob(8)"], new["blob(8)"])
    lin, dual = ctx.skin(node["blob(7)"])["device_commits"], ctx.skin_dq(node["blob(257)"])["device_commits"]
    ctx.commit_deformed()
    s, d, m = ctx.skin(node["blob(7)"]), ctx.skin_dq(node["blob(257)"]), ctx.morph(node["blob(8)"])
    assert (s["device_commits"], s["device_meshes"], s["host_meshes"]) == (lin + 1, 1, 0), "ft_debug_skin counts the matrix skin alone"
    assert (d["device_commits"], d["device_meshes"], d["host_meshes"], d["palette_kind"]) == (dual + 1, 1, 0, 2), "ft_debug_skin_dq counts the dual-quaternion skin alone"
    assert (m["device_meshes"], m["host_meshes"], m["from_device"]) == (1, 0, False)
    assert [ctx.skin_dq(node[k])["palette_kind"] for k in ("blob(7)", "blob(1025)", "blob(8)")] == [1, 0, 0]
    assert ctx.skin(node["blob(257)"])["resident_bytes"] == skin_bytes(base, 3, 20) and ctx.skin(node["blob(7)"])["resident_bytes"] == skin_bytes(b7, 2, 4, per_bone=96)
    for name in new:
        mm = ctx.morph(node[name])
        assert mm["from_device"] == (name != "blob(8)") and same(mm["scan"][:7], replay_scan(new[name])), name
    T1 = ctx.mesh_trees()
    assert_same_topology(T0, T1, "multi")
    for part, h in zip(B.MULTI_PARTS, rec2.meshes):
        if part[0] in new:
            twin.set_mesh_triangles(h, new[part[0]])
    twin.commit_deformed()
    same_trees(T1, twin.mesh_trees(), "four routes against explicit vertices")
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])


@pytest.mark.gpu
def test_the_palette_kind_switches_between_commits(contexts):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin)
    e = CAT["blob(257)"]
    base, index, weight, dq = pose_of(e, 3, 10, "mixed")
    bones = palette(10, 61, e.centre, e.radius, amount=0.5)
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    node = rec.meshes[0]
    ctx.set_mesh_skin(node, index, weight)
    fixed = skin_bytes(base, 3, 0)                                   # rest shape, index words, weights: resident once, whatever the palette
    cam, jit = B.camera(e.centre, 2.5 * e.radius), ft.jitter_pattern(SPP)
    for step, kind in enumerate((1, 2, 2, 1, 2, 0, 2)):
        before = (ctx.skin(node)["device_commits"], ctx.skin_dq(node)["device_commits"])
        if kind == 1:
            pal = palette(10, 61 + step, e.centre, e.radius, amount=0.5)
            ctx.set_mesh_bones(node, pal)
            v = ft.skin_blend(base, index, weight, pal)
        elif kind == 2:
            pal = dq_palette(10, 61 + step, e.centre, e.radius)
            ctx.set_mesh_bones_dq(node, pal)
            v = ft.skin_blend_dq(base, index, weight, pal)
        else:
            (ctx.set_mesh_bones if step % 2 else ctx.set_mesh_bones_dq)(node, np.zeros((0, 8)))
            v = base
        ctx.commit_deformed()
        s, d = ctx.skin(node), ctx.skin_dq(node)
        assert d["palette_kind"] == kind, step
        assert (s["device_commits"], d["device_commits"]) == (before[0] + (kind == 1), before[1] + (kind == 2)), step
        assert (s["device_meshes"], d["device_meshes"], s["host_meshes"], d["host_meshes"]) == (int(kind == 1), int(kind == 2), 0, 0), step
        if kind:
            assert s["resident_bytes"] == fixed + 10 * (96 if kind == 1 else 64), (step, s["resident_bytes"])
        twin.set_mesh_triangles(rec2.meshes[0], v)
        twin.commit_deformed()
        same_trees(ctx.mesh_trees(), twin.mesh_trees(), f"step {step}")
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0]), step
    assert bones.shape == (10, 12)


@pytest.mark.gpu
def test_a_zero_blend_is_refused_on_the_device_and_a_later_pose_commits(contexts):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin)
    e = CAT["blob(257)"]
    base, index, weight, dq = pose_of(e, 2, 4, "equal")
    rec, rec2 = Recorder(ctx), Recorder(twin)
    B.build_scene(rec, base)
    B.build_scene(rec2, base)
    node = rec.meshes[0]
    cam, jit = B.camera(e.centre, 2.5 * e.radius), ft.jitter_pattern(SPP)
    ctx.set_mesh_skin(node, index, weight)
    ctx.set_mesh_bones_dq(node, dq)
    ctx.commit_deformed()
    frame, T1 = ctx.render(cam, RES, RES, SPP, jit)[0], ctx.mesh_trees()
    assert (frame != frame[0, 0]).any(), "the mesh is not in the frame"
    commits = ctx.skin_dq(node)["device_commits"]
    zi, zw = _zero_blend(base.shape[0])
    zi[5:] = index[5:]                                               # some corners only: the others stay finite
    zw[5:] = weight[5:]
    ctx.set_mesh_skin(node, zi, zw)
    ctx.set_mesh_bones_dq(node, dq)
    assert ctx._lib.ft_scene_commit_deformed(ctx._ctx) == -4 and "non-finite" in ctx.last_error()
    assert counts(ctx, node) == (commits + 1, 1, 0) and ctx.morph(node)["from_device"], "the refusal did not come from the device's scan"
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], frame)
    same_trees(ctx.mesh_trees(), T1, "after the refused commit")
    dq2 = dq_palette(4, 41, e.centre, e.radius)
    ctx.set_mesh_skin(node, index, weight)                           # and no state was lost: the next pose commits
    ctx.set_mesh_bones_dq(node, dq2)
    ctx.commit_deformed()
    twin.set_mesh_triangles(rec2.meshes[0], ft.skin_blend_dq(base, index, weight, dq2))
    twin.commit_deformed()
    assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])
    same_trees(ctx.mesh_trees(), twin.mesh_trees(), "the pose after the refusal")


@pytest.mark.gpu
@pytest.mark.parametrize("retree", [0, 1])
def test_light_space_structures_follow_the_dq_bones(contexts, retree):
    ctx, twin = contexts("work"), contexts("fresh")
    _options(ctx, twin, deform_light_space=1, light_space_retree=retree)
    e = CAT["blob(257)"]
    base, index, weight, _ = pose_of(e, 2, 8, "equal")
    cam, jit = B.camera(e.centre, 2.0 * e.radius), ft.jitter_pattern(SPP)
    nodes = [_ground_scene(c, base) for c in (ctx, twin)]
    ctx.set_mesh_skin(nodes[0], index, weight)
    for seed in (1, 2):
        dq = dq_palette(8, 400 + seed, e.centre, e.radius, amount=0.5)
        v = ft.skin_blend_dq(base, index, weight, dq)
        ctx.set_mesh_bones_dq(nodes[0], dq)
        ctx.commit_deformed()
        assert ctx.morph(nodes[0])["from_device"] and counts(ctx, nodes[0])[1:] == (1, 0)
        twin.set_mesh_triangles(nodes[1], v)
        twin.commit_deformed()
        got, want = light_space(ctx), light_space(twin)
        assert got[3][0] != 0xFFFFFFFF, "the caster's leaf lost its pairs"
        for a, b, what in zip(got, want, ("pairs", "nodes and grids", "records", "leaf pairs")):
            assert same(a, b), what
        assert same(ctx.render(cam, RES, RES, SPP, jit)[0], twin.render(cam, RES, RES, SPP, jit)[0])
    _options(ctx, twin)


@pytest.mark.gpu
@pytest.mark.parametrize("follow", [0, 1])
def test_the_temporal_accumulation_follows_dq_bones_as_it_follows_vertices(contexts, follow):
    W, Hh, calls = 96, 64, 5
    e = CAT["blob(257)"]
    base, index, weight, _ = pose_of(e, 2, 5, "equal")
    jit = np.zeros((1, 2))
    cams = [B.camera(e.centre + np.array([0.05 * k, 0.0, 0.0]), 2.0 * e.radius) for k in range(calls)]
    rest = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (5, 1))

    def run(ctx, by_bones):
        m = _ground_scene(ctx, base)
        if by_bones:
            ctx.set_mesh_skin(m, index, weight)
        ctx.temporal_begin(W, Hh)
        out = []
        for k, cam in enumerate(cams):
            if k:
                dq = rest if k < 2 else dq_palette(5, 500, e.centre, e.radius, amount=0.3 * (k - 1))
                if by_bones:
                    ctx.set_mesh_bones_dq(m, dq)
                else:
                    ctx.set_mesh_triangles(m, ft.skin_blend_dq(base, index, weight, dq))
                ctx.commit_deformed()
            ctx.render(cam, W, Hh, 1, jit, seed=100 + k, fetch=False)
            ctx.temporal_accumulate(cam, 1, jit, seed=100 + k, fetch=False)
            out.append(([np.asarray(a).tobytes() for a in ctx.temporal_fetch()], ctx.temporal_status()))
        ctx.temporal_end()
        return out
    _options(contexts("work"), contexts("fresh"), temporal_follow_deformed=follow)
    explicit, bones = run(contexts("fresh"), False), run(contexts("work"), True)
    assert explicit == bones and bones[-1][1]["calls"] == calls
    _options(contexts("work"), contexts("fresh"))


@pytest.mark.gpu
def test_queued_frames_see_the_pose_they_were_queued_under(contexts):
    ctx, fresh = contexts("work"), contexts("fresh")
    _options(ctx, fresh, bvh_builder=3)
    e = CAT["blob(257)"]
    base, index, weight, dq = pose_of(e, 4, 9, "equal")
    rec = Recorder(ctx)
    B.build_scene(rec, base)
    cam, jit = B.camera(e.centre, 2.0 * e.radius), ft.jitter_pattern(SPP)
    old = ctx.render(cam, RES, RES, SPP, jit)[0]
    ctx.set_mesh_skin(rec.meshes[0], index, weight)
    for _ in range(2):
        ctx.render_enqueue(cam, RES, RES, SPP, jit)
    ctx.set_mesh_bones_dq(rec.meshes[0], dq)
    ctx.commit_deformed()                                            # retires the queued frames first: they traced the old pose
    assert same(ctx.fetch_frame(np.zeros((RES, RES, 3))), old), "the last frame queued before the commit is not the old pose's"
    ctx.render_enqueue(cam, RES, RES, SPP, jit)
    ctx.wait()
    B.build_scene(fresh, ft.skin_blend_dq(base, index, weight, dq))
    new = fresh.render(cam, RES, RES, SPP, jit)[0]
    assert not same(new, old)
    assert same(ctx.fetch_frame(np.zeros((RES, RES, 3))), new), "a frame queued after the commit is not the new pose's"
    _options(ctx, fresh)


@pytest.mark.gpu
def test_every_device_of_a_context_skins_its_copy(contexts):
    one = contexts("work")
    _options(one, bvh_builder=3)
    two = ft.Context(device=[0, 0])
    try:
        two.set_option("bvh_builder", 3)
        e = CAT["blob(257)"]
        base, index, weight, dq = pose_of(e, 4, 30, "mixed")
        view = view_of(ft.skin_blend_dq(base, index, weight, dq))
        out = []
        for c in (one, two):
            rec = Recorder(c)
            B.build_scene(rec, base)
            c.set_mesh_skin(rec.meshes[0], index, weight)
            c.set_mesh_bones_dq(rec.meshes[0], dq)
            c.commit_deformed()
            assert c.morph(rec.meshes[0])["from_device"] and counts(c, rec.meshes[0])[1:] == (1, 0)
            out.append((c.render(B.camera(*view), RES, RES, SPP, ft.jitter_pattern(SPP))[0], c.mesh_trees()))
        assert same(out[0][0], out[1][0]), "the two devices' bands are not the single device's frame"
        same_trees(out[0][1], out[1][1], "two devices")
    finally:
        two.close()
        _options(one)

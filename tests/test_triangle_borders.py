"""tri_hit and tri_hit_wave (ft_kernels.hip) on edges, vertices and their epsilon borders, bit for bit against a reference in plain floats
(tests/tri_tools.py).

Family A: lattice meshes under a lattice camera - pixel rays run exactly through vertices (hubs of 4 to 8 triangles), along points of
shared edges and hypotenuses, through interiors and one pixel outside the rim; a sheet in both windings, a mesh of coincident
duplicates, a fan, and gapped sheets that BspMesh.compile cuts at depths 1 to 3 without clipping a triangle.
Family B: the ulp band around u = 1, v = 1, u + v = 1, u = 0, v = 0 on axis-aligned triangles with a 53-bit edge.
Family C: |a| and t at pred(eps), eps, succ(eps), d scaled by 2^-24 .. 2^24, max_dist at pred(t), t, succ(t), hits behind the origin, a
degenerate triangle.

The CPU half asserts that the guard keeps every ray, that the reference is right on hand-worked rays, that the oracle equals it bit for
bit on every family, and that the meshes build as meant on a host-only context.  The GPU half asserts the same of the device: through
render_aov (k_aov: the coherent walks and the candidate lists), through frames (k_primary, k_primary_mesh: twins bitwise equal, the hit
counter equal to the reference's) and through closest / blocked (the per-lane walks and the linear scans)."""
import functools
import math

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from . import tri_tools as T

gpu = pytest.mark.gpu
W, Hh = T.RES_H, T.RES_V
JITTER = np.array(T.OFFSETS)
LATTICE = ["sheet", "duplicates", "fan"]
GAPPED = [("gapped", d) for d in T.BSP_DEPTHS]
EYES = {"near": T.NEAR, "big": T.BIG}
# What `options` puts back into the session's shared context: the initial values of the Options struct in functracer_amd/csrc/ft_context.h
# (coherent_waves, classify_pixels, bvh_builder, primary_block_lists, primary_mesh_kernel, edge_cull) and of light_space_shadows in
# ft_scene.h, as include/functracer_hip.h documents them ("1 = default", "2 = default").  The ABI has no getter; a default that changes
# there changes here.
DEFAULTS = {"coherent_waves": 1, "primary_block_lists": 1, "edge_cull": 1, "bvh_builder": 2, "classify_pixels": 1, "primary_mesh_kernel": 1, "light_space_shadows": 2}


def mesh_id(m):
    return m if isinstance(m, str) else f"gapped{m[1]}"


def depth_of(m):
    return 0 if isinstance(m, str) else m[1]


# =============================================================================================================================
# CPU half

def test_reference_on_hand_worked_rays():
    """v0 = (0, 0, 0), v1 = (2, 0, 0), v2 = (0, 4, 0) seen along -z from z = 3: a = 8, u = x / 2, v = y / 4, t = 3."""
    tri = ((0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 4.0, 0.0))
    down = (0.0, 0.0, -1.0)
    at = lambda x, y, T_=tri, d=down, z=3.0: T.tri_reference(T_, (x, y, z), d)
    assert at(0.0, 0.0) == (True, 3.0, 0.0, 0.0)                        # through each vertex
    assert at(2.0, 0.0) == (True, 3.0, 1.0, 0.0)
    assert at(0.0, 4.0) == (True, 3.0, 0.0, 1.0)
    assert at(1.0, 0.0) == (True, 3.0, 0.5, 0.0)                        # the edge midpoints
    assert at(0.0, 2.0) == (True, 3.0, 0.0, 0.5)
    assert at(1.0, 2.0) == (True, 3.0, 0.5, 0.5)                        # ... of the hypotenuse: u + v == 1
    assert at(0.5, 1.0) == (True, 3.0, 0.25, 0.25)                      # an interior point
    step = 1.0 / 8                                                      # outside by one lattice step
    assert at(-step, 1.0)[0] is False and at(1.0, -step)[0] is False and at(1.0 + step, 2.0)[0] is False and at(2.0 + step, 0.0)[0] is False
    assert at(1.0, 2.0 + step)[:2] == (False, None)
    back = (tri[0], tri[2], tri[1])                                     # the other winding: a = -8, u and v change places
    assert T.tri_reference(back, (0.5, 1.0, 3.0), down) == (True, 3.0, 0.25, 0.25)
    assert T.tri_reference(back, (2.0, 0.0, 3.0), down) == (True, 3.0, 0.0, 1.0)
    assert T.tri_reference(tri, (0.5, 1.0, -3.0), (0.0, 0.0, 1.0)) == (True, 3.0, 0.25, 0.25)   # from below: a = -8 as well
    assert T.tri_reference(tri, (0.5, 1.0, -3.0), down) == (False, -3.0, 0.25, 0.25)            # behind the origin
    assert T.tri_reference(tri, (0.5, 1.0, 3.0), (1.0, 0.0, 0.0))[0] is False                    # in the plane: a == 0
    # a tilted triangle under a slanted ray, worked by hand: e1 = (2, 0, 1), e2 = (0, 2, 2), d = (0, 1, -1): h = d x e2 = (4, 0, 0), a = 8;
    # s = (1, 1, 3): s.h = 4, u = 1/2; q = s x e1 = (1, 5, -2), d.q = 7, v = 7/8: outside.  s = (1/2, 1/4, 3): u = 1/4; q = (1/4, 11/2, -1/2),
    # d.q = 6, v = 3/4: on the hypotenuse; e2.q = 10, t = 5/4, and o + t d = (1/2, 3/2, 7/4) = v0 + e1 / 4 + 3 e2 / 4
    tilt = ((0.0, 0.0, 0.0), (2.0, 0.0, 1.0), (0.0, 2.0, 2.0))
    assert T.tri_reference(tilt, (1.0, 1.0, 3.0), (0.0, 1.0, -1.0)) == (False, None, 0.5, 0.875)
    assert T.tri_reference(tilt, (0.5, 0.25, 3.0), (0.0, 1.0, -1.0)) == (True, 1.25, 0.25, 0.75)
    third = ((0.0, 0.0, 0.0), (3.0, 0.0, 1.0), (0.0, 2.0, 2.0))         # a = 12: the division's rounding stays in u, v and t
    f = 1.0 / 12.0
    assert T.tri_reference(third, (0.75, 0.25, 3.0), (0.0, 1.0, -1.0)) == (True, f * 15.0, f * 3.0, f * 9.0)
    # the vectorised form is the scalar one
    rng = np.random.default_rng(3)
    tris = rng.integers(-8, 9, size=(40, 3, 3)) / 4.0
    o, dd = rng.integers(-16, 17, size=(50, 3)) / 8.0, rng.integers(-8, 9, size=(50, 3)) / 8.0
    hit_g, t_g = T.tri_reference_grid(tris, o, dd)
    n_hit = 0
    for i in range(50):
        for j in range(40):
            hit, t, _, _ = T.tri_reference(tris[j], o[i], dd[i])
            assert hit == hit_g[i, j] and (not hit or t == t_g[i, j])
            n_hit += hit
    assert n_hit > 20


def test_guard_on_hand_cases():
    tri = ((0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 4.0, 0.0))
    assert T.exact_guard(tri, (0.5, 1.0, 3.0), (0.0, 0.0, -1.0))
    assert not T.exact_guard(tri, (0.1, 1.0, 3.0), (0.3, 0.0, -1.0))      # 0.1 * 0.3-like products are no doubles
    third = ((0.0, 0.0, 0.0), (1.0 / 3.0, 0.0, 0.0), (0.0, 0.5, 0.0))
    assert not T.exact_guard(third, (0.1, 0.1, 1.0), (0.0, 0.0, -1.0))   # a 53-bit edge times a 53-bit offset
    assert T.exact_guard(third, (1.0 / 3.0, 0.25, 1.0), (0.0, 0.0, -1.0))   # ... times a power of two is one
    assert T.representable(T.F(1, 2 ** 1074)) and not T.representable(T.F(1, 3)) and not T.representable(T.F(2 ** 53 + 1))


def test_lattice_camera_is_exact():
    """The plane and the rays as the module docstring of tri_tools states them, against the oracle's; slightOffset is absorbed at BIG."""
    for name, eye in EYES.items():
        cam = T.camera(eye)
        ip = O.image_plane(cam, W, Hh)
        assert ip["i"].tolist() == [-1, 0, 0] and ip["j"].tolist() == [0, 1, 0] and ip["k"].tolist() == [0, 0, -1]
        assert (ip["pixel_width"], ip["pixel_height"], ip["top_left"][0], ip["top_left"][1]) == (float(T.PW), float(T.PH), float(T.TLX), float(T.TLY))
        o, d, d_i, xs, ys, ks = T.lattice_rays(name)
        for k in range(0, len(o), 7):
            oo, dd = O.ray_through_pixel(cam, W, Hh, int(xs[k]), int(ys[k]), *T.OFFSETS[ks[k]])
            assert np.array_equal(oo, o[k]) and np.array_equal(dd, d[k]), (name, k)
    assert T.pixel_dir(0, 0, 0.25, -0.5) == (T.F(61, 64), T.F(31, 64), -1)
    assert T.pixel_dir(15, 31, 0.5, -0.5) == (0, 0, -1)
    o, d, *_ = T.lattice_rays("big")
    assert np.array_equal(o + T.SLIGHT * d, o), "two roundings"
    c = T.F(T.SLIGHT)
    for ro, rd in zip(o[::5], d[::5]):
        assert [float(T.F(a) + c * T.F(b)) for a, b in zip(ro, rd)] == ro.tolist(), "one rounding (a fused multiply-add)"
    o, d, *_ = T.lattice_rays("near")
    assert not np.array_equal(o + T.SLIGHT * d, o)


@pytest.mark.parametrize("mesh", LATTICE + GAPPED, ids=mesh_id)
def test_guard_keeps_every_lattice_ray(mesh):
    """100 % of rays x triangles; the floats the reference forms are the exact integers; the Fraction guard agrees on a sample; the model
    frame of the transformed twin passes as well."""
    for eye in EYES:
        A = T.lattice_answers(mesh, eye)
        assert A["kept"].all(), f"{mesh_id(mesh)}/{eye}: the guard drops {int((~A['kept']).sum())} of {A['kept'].size}"
    o, d, d_i, xs, ys, ks = T.lattice_rays("big")
    tris = A["tris"].reshape(-1, 3, 3)
    a_i = A["exact"][0]
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    rows = np.arange(0, len(o), 11)
    D = d[rows, None, :]
    h = np.stack([D[..., 1] * e2[None, :, 2] - D[..., 2] * e2[None, :, 1], D[..., 2] * e2[None, :, 0] - D[..., 0] * e2[None, :, 2], D[..., 0] * e2[None, :, 1] - D[..., 1] * e2[None, :, 0]], axis=-1)
    a_f = (e1[None] * h).sum(axis=-1)
    assert np.array_equal(a_f * (T.D_SCALE * T.V_SCALE * T.V_SCALE), a_i[rows].astype(np.float64))
    rng = np.random.default_rng(5)
    for _ in range(150):
        i, j = int(rng.integers(len(o))), int(rng.integers(len(tris)))
        assert T.exact_guard(tris[j], o[i], d[i])
    stretch = np.array([2, 8, 1], dtype=np.int64)                      # 4 / (2, 1/2, 4): the model frame under tri_tools.transform_ops
    kept = T.lattice_guard(A["rel"] * stretch, np.zeros_like(d_i), d_i * stretch)[0]
    assert kept.all()


def test_families_hold_their_borders():
    """What the sheet's rays are there for, counted on the reference."""
    A = T.lattice_answers("sheet", "big")
    o, d, d_i, xs, ys, ks = T.lattice_rays("big")
    n_hits = A["hit_grid"].sum(axis=1)
    first = ks == 0
    even = first & (xs % 2 == 0) & (ys % 2 == 0) & (xs >= 10) & (xs <= 54) & (ys >= 6) & (ys <= 26)
    assert even.sum() > 200 and (n_hits[even] >= 4).all() and (n_hits[even] == 8).any(), "interior vertices are hubs of 4 and 8 triangles"
    on_edge = first & ((xs % 2 == 1) ^ (ys % 2 == 1)) & (xs > 8) & (xs < 56) & (ys > 4) & (ys < 28)
    assert (n_hits[on_edge] == 2).mean() > 0.9, "rays through the points of shared edges hit both triangles"
    diag = first & (xs % 2 == 1) & (ys % 2 == 1) & (xs > 8) & (xs < 56) & (ys > 4) & (ys < 28)
    assert (n_hits[diag] == 2).mean() > 0.9, "rays through the midpoints of quads hit both triangles of the hypotenuse"
    rim_out = first & ((xs == 7) | (xs == 57) | (ys == 3) | (ys == 29))
    assert rim_out.sum() > 100 and not A["hit"][rim_out].any()
    rim = first & (xs == 8) & (ys >= 4) & (ys <= 28)
    assert A["hit"][rim].all(), "the rim itself is hit"
    inner = (ks == 3) & (xs > 8) & (xs < 56) & (ys > 4) & (ys < 28)
    assert (n_hits[inner] >= 1).all() and (n_hits[inner] == 1).mean() > 0.5 and (n_hits[inner] == 2).any(), "the quarter-pixel offset: interiors, and points of the diagonals"
    tied = n_hits >= 2
    spread = np.zeros(len(n_hits))
    spread[tied] = np.where(A["hit_grid"], A["t_grid"], -np.inf)[tied].max(axis=1) - np.where(A["hit_grid"], A["t_grid"], np.inf)[tied].min(axis=1)
    print(f"\n  sheet: {int(tied.sum())} rays hit 2 .. 8 triangles; their t agree bit for bit on {int((spread[tied] == 0).sum())}, differ by an ulp or two on {int((spread[tied] > 0).sum())}")
    assert (spread[tied] < 1e-14).all() and (spread[tied] == 0).any()
    assert (d[:, 0] == 0).sum() >= 32 and ((d[:, 0] == 0) & A["hit"]).sum() >= 12, "a pixel column with jx == 0"
    dup = T.lattice_answers("duplicates", "big")
    assert dup["hit"].sum() > 1000 and (dup["winner"][dup["hit"]] % 2 == 0).all(), "of two coincident triangles the first wins"
    fan = T.lattice_answers("fan", "big")
    hub = (ks == 0) & (xs == 32) & (ys == 16)
    assert fan["hit_grid"][hub].sum() == 8 and fan["winner"][hub][0] == 0
    signs = np.sign(A["exact"][0][0])
    assert (signs > 0).sum() > 200 and (signs < 0).sum() > 200, "both windings: both signs of a"


@functools.lru_cache(maxsize=None)
def oracle():
    return O.Oracle()


def _max_dists(A):
    """pred(t), t, succ(t) and no bound in turn on the rays that hit, no bound on the others."""
    t = A["t"]
    md = np.full(len(t), 1e300)
    idx = np.nonzero(A["hit"])[0]
    for k, fn in enumerate((lambda v: np.nextafter(v, 0.0), lambda v: v, lambda v: np.nextafter(v, np.inf))):
        sel = idx[k::4]
        md[sel] = fn(t[sel])
    return md


def check_rays(b, A, o, d, what, winner=None, normals=False):
    """closest and blocked of builder b (the oracle or the device) on explicit rays against the reference: hit and t bit for bit; the
    winner where the scene's colours name it; with `normals` the winner's plane."""
    hit, t, p, n, col = b.closest(o, d)
    want = A["hit"]
    assert np.array_equal(hit.astype(bool), want), f"{what}: hit / miss differs on rays {np.nonzero(hit.astype(bool) != want)[0][:8]}"
    bad = np.nonzero(want & (t != A["t"]))[0]
    assert bad.size == 0, f"{what}: t differs on {bad.size} rays, first {bad[:5]}: {t[bad[:3]]!r} vs {A['t'][bad[:3]]!r}"
    if winner is not None:
        got = T.colour_index(col[want])
        assert np.array_equal(got, winner[want]), f"{what}: another triangle wins on {int((got != winner[want]).sum())} rays"
    if normals:
        tr = A["tris"].reshape(-1, 3, 3)[A["winner"][want]]
        nn = np.cross(tr[:, 1] - tr[:, 0], tr[:, 2] - tr[:, 0])
        nn /= np.linalg.norm(nn, axis=1)[:, None]
        assert np.abs(np.abs((nn * n[want]).sum(axis=1)) - 1.0).max() < 1e-9, f"{what}: the normal is not the reference winner's"
    md = _max_dists(A)
    got = b.blocked(o, d, md).astype(bool)
    ref = T.blocked_reference(A["hit_grid"], A["t_grid"], md)
    assert np.array_equal(got, ref), f"{what}: blocked differs on rays {np.nonzero(got != ref)[0][:8]}"
    assert ref.any() and (want & ~ref).any(), f"{what}: the max_dist borders show both outcomes"


def lattice_scenes(mesh, eye_name):
    """name -> (lower, winner known by colour, normals decide) for the explicit-ray checks of a lattice mesh."""
    A, eye, depth = T.lattice_answers(mesh, eye_name), EYES[eye_name], depth_of(mesh)
    out = {"mesh": (T.lower_mesh(A["tris"], depth, eye=eye), False), "csg": (T.lower_csg(A["tris"], depth, eye=eye), False)}
    if depth == 0:
        out["group"] = (T.lower_group(A["tris"]), True)
        ops = T.transform_ops(eye)
        out["transformed"] = (T.lower_mesh(T.vertices(A["rel"], eye, ops), 0, ops=ops, eye=eye), False)
    return A, out


@pytest.mark.parametrize("eye", list(EYES))
@pytest.mark.parametrize("mesh", LATTICE + GAPPED, ids=mesh_id)
def test_oracle_equals_reference_on_lattice_rays(mesh, eye):
    A, scenes = lattice_scenes(mesh, eye)
    o, d, *_ = T.lattice_rays(eye)
    for name, (lower, by_colour) in scenes.items():
        lower(oracle())
        check_rays(oracle(), A, o, d, f"{mesh_id(mesh)}/{eye}/{name}", winner=A["winner"] if by_colour else None, normals=depth_of(mesh) == 0 and mesh != "duplicates")


# ---- Family B
@functools.lru_cache(maxsize=None)
def band(A, subnormal=False):
    """The band's cases without the subnormal steps around u = 0 / v = 0, or those alone."""
    cases = [c for c in T.band_cases(A) if c[0].startswith("zero_tiny") == subnormal]
    ref = [T.tri_reference(c[1], c[2], c[3]) for c in cases]
    return cases, ref


def _by_triangle(cases, ref):
    groups = {}
    for c, r in zip(cases, ref):
        groups.setdefault(c[1], []).append((c, r))
    return groups


@pytest.mark.parametrize("A", T.B_SIZES)
def test_band_is_guarded_and_has_content_on_both_sides(A):
    cases, ref = [x + y for x, y in zip(band(A), band(A, True))]
    assert all(T.exact_guard(c[1], c[2], c[3]) for c in cases), "the guard drops a ray of the band"
    f = 1.0 / A
    assert any(f * T.step(A, k) <= 1.0 for k in range(1, 25)), "no k >= 1 that the reference still hits"
    early = [k for k in range(1, 25) if T.step(A, k) > A * T.REJECT]
    late = [k for k in range(1, 25) if T.step(A, k) <= A * T.REJECT and f * T.step(A, k) > 1.0]
    assert late, "the band holds no miss below the early reject"
    by = {}
    for c, r in zip(cases, ref):
        by.setdefault(c[0], []).append((c[4], r[0]))
    for label, rows in by.items():
        hits = [k for k, h in rows if h]
        misses = [k for k, h in rows if not h]
        assert hits and misses, f"{label}: one outcome only"
        if label.startswith("one"):
            assert max(hits) >= 1 and any(1 <= k <= max(late) for k in misses), label
        if label.startswith("zero"):
            # u = f * sh of a subnormal sh can round to -0, which is not < 0: the reference then hits one step outside (Triangle.fs:54)
            assert min(hits) in (0, -1) and max(misses) < 0, label
    print(f"\n  A = {A!r}: u = 1 still hit up to k = {max(k for k in range(0, 25) if f * T.step(A, k) <= 1.0)}, missed by the division from k = {min(late)}, by the early reject from k = {min(early) if early else '> 24'}")


def small_scenes(tris, filler):
    t = T.with_filler(tris) if filler else np.array([np.array(x, dtype=np.float64).reshape(9) for x in tris])
    return t


def check_small(b, tri_list, rows, what, kinds=("scan", "bvh", "group", "csg", "bsp")):
    """One small triangle set through every per-lane path of builder b: rows = [(o, d, (hit, t), max_dists or None)], the expectation
    per ray being the closest over tri_list (a single triangle, or the degenerate pair).  "bsp" is a `bspMesh 1`: its branch box
    (BoundingBox.fs:32-58) stands in front of the triangle test, and these rays run along the box's faces with zero direction components
    (0 * inf, NaN comparisons), so the box and not Triangle.fs decides some of them: there the expectation is the oracle's answer, and the
    oracle itself is not checked."""
    o = np.array([r[0] for r in rows])
    d = np.array([r[1] for r in rows])
    want_hit = np.array([r[2][0] for r in rows])
    want_t = np.array([r[2][1] if r[2][0] else np.inf for r in rows])
    lowers = {"scan": T.lower_mesh(small_scenes(tri_list, False), 0, light=False), "bvh": T.lower_mesh(small_scenes(tri_list, True), 0, light=False),
              "bsp": T.lower_mesh(small_scenes(tri_list, True), 1, light=False), "group": T.lower_group(small_scenes(tri_list, False)),
              "csg": T.lower_csg(small_scenes(tri_list, False), 0)}
    for kind in kinds:
        if kind == "bsp":
            if b is oracle():
                continue
            lowers[kind](oracle())
            oh, ot, _, _, _ = oracle().closest(o, d)
            want_hit, want_t = oh.astype(bool), np.where(oh.astype(bool), ot, np.inf)
        lowers[kind](b)
        hit, t, _, _, _ = b.closest(o, d)
        bad = np.nonzero(hit.astype(bool) != want_hit)[0]
        assert bad.size == 0, f"{what}/{kind}: hit / miss differs on rays {bad[:6]} (o = {o[bad[:2]].tolist()})"
        bad = np.nonzero(want_hit & (t != want_t))[0]
        assert bad.size == 0, f"{what}/{kind}: t differs on rays {bad[:6]}: {t[bad[:3]]!r} vs {want_t[bad[:3]]!r}"
        md = np.array([np.inf if not h else (np.nextafter(tt, 0.0), tt, np.nextafter(tt, np.inf))[i % 3] for i, (h, tt) in enumerate(zip(want_hit, want_t))])
        for i, r in enumerate(rows):
            if r[3] is not None:
                md[i] = r[3]
        md = np.where(np.isinf(md), 1e300, md)
        got = b.blocked(o, d, md).astype(bool)
        ref = want_hit & (want_t < md)
        assert np.array_equal(got, ref), f"{what}/{kind}: blocked differs on rays {np.nonzero(got != ref)[0][:6]}"


@pytest.mark.parametrize("A", T.B_SIZES)
def test_oracle_equals_reference_on_the_band(A):
    cases, ref = [x + y for x, y in zip(band(A), band(A, True))]
    for tri, rows in _by_triangle(cases, ref).items():
        check_small(oracle(), [tri], [(c[2], c[3], (r[0], r[1]), None) for c, r in rows], f"A={A!r}/{rows[0][0][0]}")


# ---- Family C
def eps_rows():
    rows = {}
    for label, tri, o, d, mds in T.eps_cases():
        r = T.tri_reference(tri, o, d)
        assert T.exact_guard(tri, o, d), label
        for md in (mds or (None,)):
            rows.setdefault(tri, []).append((o, d, (r[0], r[1]), md, label))
    return rows


def test_epsilon_cases_are_what_their_names_say():
    got = {label: T.tri_reference(tri, o, d) for label, tri, o, d, _ in T.eps_cases()}
    assert [got[k][0] for k in ("a=pred", "a=eps", "a=succ", "a=-pred", "a=-eps", "a=-succ")] == [False, True, True, False, True, True]
    assert got["a=pred"][2] is None and got["a=-pred"][2] is None, "rejected by the near-parallel test itself"
    scaled = [got[f"d*2^{e}"][0] for e in range(-24, 25, 2)]
    assert scaled == [False] * 6 + [True] * 19, "the near-parallel reject depends on |d|"
    assert [got[f"d*2^{e}/flip"][0] for e in range(-24, 25, 2)].count(False) in range(1, 12)
    assert [got[k][0] for k in ("t=pred", "t=eps", "t=succ", "t=behind", "t=at")] == [False, False, True, False, False]
    assert got["t=succ"][1] == math.nextafter(T.EPS, 1.0) and got["t=behind"][1] == -1.0
    assert got["max_dist/t=0.7"][:2] == (True, 0.7)
    for tri in T.DEGENERATE[:1]:
        assert T.tri_reference(tri, (0.5, 0.0, 1.0), (0.0, 0.0, -1.0))[:2] == (False, None)


def degenerate_rows():
    rays = [((x / 4.0, y / 4.0, 1.0), (0.0, 0.0, -1.0)) for x in range(-1, 10) for y in range(-1, 6)]
    rows = []
    for o, d in rays:
        r = [T.tri_reference(tri, o, d) for tri in T.DEGENERATE]
        assert all(T.exact_guard(tri, o, d) for tri in T.DEGENERATE)
        assert not r[0][0]
        rows.append((o, d, (r[1][0], r[1][1]), None))
    assert sum(r[2][0] for r in rows) >= 10 and sum(not r[2][0] for r in rows) >= 10
    return rows


def test_oracle_equals_reference_on_the_epsilon_cases():
    for tri, rows in eps_rows().items():
        check_small(oracle(), [tri], [r[:4] for r in rows], rows[0][4])
    check_small(oracle(), T.DEGENERATE, degenerate_rows(), "degenerate")


# ---- a host-only context commits every scene, and the trees are what the tests take them for
def test_host_only_context_commits_every_scene():
    ctx = ft.Context(host_only=True)
    try:
        for mesh in LATTICE + GAPPED:
            for eye_name, eye in EYES.items():
                A, scenes = lattice_scenes(mesh, eye_name)
                for name, (lower, _) in scenes.items():
                    lower(ctx)
                    if name == "transformed":
                        w2m = ctx.leaf_matrices()[1][0]
                        s, tr = [T.F(c) for c in T.transform_ops(eye)[0][1]], [T.F(c) for c in T.transform_ops(eye)[1][1]]
                        want = np.zeros((3, 4))
                        for k in range(3):
                            want[k, k], want[k, 3] = float(1 / s[k]), float(-tr[k] / s[k])
                        assert np.array_equal(w2m, want), "the composed world-to-model matrix is exact"
                tris = A["tris"].reshape(-1, 3, 3)
                T.lower_mesh(A["tris"], depth_of(mesh), eye=eye)(ctx)
                M = ctx.mesh_trees()
                want = np.concatenate([tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]], axis=1)
                src = M["tri_src"]
                assert np.array_equal(M["tris"], want[src]), f"{mesh_id(mesh)}: the tree's triangle records are not the input's, bit for bit"
                root, bvh_root = int(M["meshes"][0][0]), int(M["meshes"][0][1])
                if depth_of(mesh) == 0:
                    assert root < 0 and bvh_root >= 0, "a top-level leaf with a BVH"
                else:                                                   # one record per input triangle: nothing was clipped
                    assert M["tris"].shape[0] == len(tris) and sorted(src) == list(range(len(tris))), f"{mesh_id(mesh)}: BspMesh.compile clipped a triangle"
                    assert root >= 0 and len(M["bsp_leaves"]) == 2 ** depth_of(mesh), "a BSP of the full depth"
                T.lower_mesh(A["tris"], depth_of(mesh), eye=eye, floor=True)(ctx)
                T.lower_mesh(A["tris"], depth_of(mesh), eye=eye, beside=True)(ctx)
        tri = T.band_triangle(3.0, 1.0, 0, False)
        for kind, filler, depth in (("scan", False, 0), ("bvh", True, 0), ("bsp", True, 1)):
            T.lower_mesh(small_scenes([tri], filler), depth, light=False)(ctx)
            M = ctx.mesh_trees()["meshes"][0]
            assert (int(M[0]) < 0, int(M[1]) >= 0) == {"scan": (True, False), "bvh": (True, True), "bsp": (False, False)}[kind], (kind, M)
        T.lower_group(small_scenes([tri], False))(ctx)
        T.lower_csg(small_scenes([tri], False))(ctx)
        T.lower_mesh(axial_triangles([tri]), 0)(ctx)
    finally:
        ctx.close()


# =============================================================================================================================
# GPU half

class options:
    """Set options for a block and put the defaults back."""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


VARIANTS = {                                                            # name -> (options, beside, transformed)
    "shipped": ({}, False, False), "coherent_waves=0": ({"coherent_waves": 0}, False, False), "primary_block_lists=0": ({"primary_block_lists": 0}, False, False),
    "edge_cull=0": ({"edge_cull": 0}, False, False), "classify_pixels=0": ({"classify_pixels": 0}, False, False), "primary_mesh_kernel=0": ({"primary_mesh_kernel": 0}, False, False),
    "bvh_builder=0": ({"bvh_builder": 0}, False, False), "bvh_builder=1": ({"bvh_builder": 1}, False, False), "bvh_builder=3": ({"bvh_builder": 3}, False, False),
    "beside": ({}, True, False), "transformed": ({}, False, True),
}


def lower_variant(A, mesh, beside, transformed):
    if transformed:
        ops = T.transform_ops(T.BIG)
        return T.lower_mesh(T.vertices(A["rel"], T.BIG, ops), depth_of(mesh), ops=ops, eye=T.BIG, beside=beside)
    return T.lower_mesh(A["tris"], depth_of(mesh), eye=T.BIG, beside=beside)


def reference_planes(A):
    o, d, d_i, xs, ys, ks = T.lattice_rays("big")
    return T.as_planes(A["t"], xs, ys, ks, np.inf), T.as_planes(A["winner"].astype(np.int32), xs, ys, ks, -1)


def check_aov(ctx, A, what, winner=True):
    """render_aov of every sample offset against the reference: t bit for bit and the winning triangle on every tile pixel."""
    t_ref, w_ref = reference_planes(A)
    cam = T.camera(T.BIG)
    inside = np.zeros((Hh, W), dtype=bool)
    inside[:32, :64] = True
    for k in range(len(T.OFFSETS)):
        got = ctx.render_aov(cam, W, Hh, len(T.OFFSETS), JITTER, sample=k, tiles=T.TILES, channels=["t", "triangle"])
        bad = np.argwhere(inside & (got["t"] != t_ref[k]))
        assert bad.size == 0, f"{what}, offset {T.OFFSETS[k]}: t differs on {len(bad)} pixels, first (y, x) {bad[:4].tolist()}: {[got['t'][y, x] for y, x in bad[:3]]!r} vs {[t_ref[k][y, x] for y, x in bad[:3]]!r}"
        if winner:
            bad = np.argwhere(inside & (got["triangle"] != w_ref[k]))
            assert bad.size == 0, f"{what}, offset {T.OFFSETS[k]}: another triangle wins on {len(bad)} pixels, first (y, x) {bad[:4].tolist()}"


# the transformed twin exists at depth 0 only: the model frame is stretched per axis, BspMesh.compile cuts other planes there, and clips
AOV_CASES = [(m, v) for m in LATTICE + GAPPED for v in VARIANTS if not (VARIANTS[v][2] and depth_of(m))]


@gpu
@pytest.mark.parametrize("mesh,variant", AOV_CASES, ids=[f"{mesh_id(m)}-{v}" for m, v in AOV_CASES])
def test_aov_planes_equal_the_reference(hip, mesh, variant):
    """k_aov: mesh_bvh_packet / mesh_list_closest (bspMesh 0), mesh_bsp_packet / mesh_bsp_narrow (depths 1 .. 3), their per-lane twins
    with coherent_waves = 0.  At depth >= 1 the BSP order decides ties between triangles: t alone is compared there."""
    opts, beside, transformed = VARIANTS[variant]
    A = T.lattice_answers(mesh, "big")
    with options(hip, **opts):
        lower_variant(A, mesh, beside, transformed)(hip)
        check_aov(hip, A, f"{mesh_id(mesh)}/{variant}", winner=depth_of(mesh) == 0)


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}


@gpu
@pytest.mark.parametrize("mesh", LATTICE + GAPPED, ids=mesh_id)
def test_frames_count_the_reference_hits_and_twins_are_bitwise_equal(hip, mesh):
    """k_primary_mesh and k_primary under every option twin: one frame, bit for bit, whose primary hit counter is the reference's hit
    count over all tile pixels and offsets; the launch counters say which kernel ran, the lists' readback that lists were built and
    that the device's image plane is the exact one."""
    A = T.lattice_answers(mesh, "big")
    cam = T.camera(T.BIG)
    want_hits = int(A["hit"].sum())
    frames = {}
    for variant, (opts, beside, transformed) in VARIANTS.items():
        if transformed and depth_of(mesh):
            continue                                                    # see test_aov_planes_equal_the_reference
        with options(hip, **opts):
            lower_variant(A, mesh, beside, transformed)(hip)
            before = hip.primary_kernels()
            frame, st = hip.render(cam, W, Hh, len(T.OFFSETS), JITTER, tiles=T.TILES)
            after = hip.primary_kernels()
            assert st["hits_primary"] == want_hits, f"{mesh_id(mesh)}/{variant}: {st['hits_primary']} primary hits, the reference has {want_hits}"
            took_mesh = after["k_primary_mesh"] - before["k_primary_mesh"]
            took_generic = after["k_primary"] - before["k_primary"]
            if variant == "shipped" and depth_of(mesh) == 0:
                assert took_mesh > 0 and took_generic == 0, f"{mesh_id(mesh)}/{variant}: k_primary_mesh {took_mesh}, k_primary {took_generic}"
            if variant in ("primary_mesh_kernel=0", "coherent_waves=0", "beside") or depth_of(mesh):
                assert took_mesh == 0 and took_generic > 0, f"{mesh_id(mesh)}/{variant}: k_primary_mesh {took_mesh}, k_primary {took_generic}"
            if variant in ("shipped", "edge_cull=0", "transformed") and depth_of(mesh) == 0:
                L = hip.block_lists()
                assert L["leaf"] >= 0, f"{variant}: the frame carried no lists"
                assert L["plane"].tolist() == [float(T.TLX), float(T.TLY), float(T.PW), float(T.PH)], "the device's image plane is the exact one"
            if variant == "primary_block_lists=0":
                assert hip.block_lists()["leaf"] == -1
            frames[variant] = (frame, counters(st), beside)
    base = frames["shipped"][0]
    assert np.isfinite(base).all() and (base[:32, :64].sum(axis=2) > 0).any()
    for variant, (frame, st, beside) in frames.items():
        if variant == "transformed":                                    # shaded in another model frame: other roundings of p and n; its hits were counted above
            continue
        assert np.array_equal(frame, base), f"{mesh_id(mesh)}/{variant}: the frame differs from the shipped one on {int(np.any(frame != base, axis=2).sum())} pixels"


@gpu
def test_classification_is_reused_on_the_lattice_view(hip):
    A = T.lattice_answers("sheet", "big")
    T.lower_mesh(A["tris"], 0, eye=T.BIG)(hip)
    cam = T.camera(T.BIG)
    before = hip.classify_reuse()
    frames = [hip.render(cam, W, Hh, len(T.OFFSETS), JITTER, tiles=T.TILES)[0] for _ in range(8)]
    after = hip.classify_reuse()
    assert after["reused"] > before["reused"] and after["classified"] > before["classified"]
    assert all(np.array_equal(f, frames[0]) for f in frames)
    check_aov(hip, A, "sheet after reused classifications")


@gpu
@pytest.mark.parametrize("mesh", ["sheet", ("gapped", 2)], ids=mesh_id)
def test_shadowed_frames_against_the_oracle_and_light_space_twins(hip, mesh):
    """The near eye, a floor and a directional light.  Here the primary rays start at o + 1e-4 d and the shadow rays at p + 1e-4 n: no
    dyadic numbers, so a ray aimed at an edge or a vertex is decided by the last bit of s . h, which a fused and an unfused evaluation
    round differently (measured under OFFSETS: 249 of 2145 pixels off the oracle's on the sheet, 255 at depth 2).  The border rays are held exactly
    by the AOV planes and the hit counters at the far eye; this frame takes offsets that keep every ray an eighth of a pixel off every
    lattice line and diagonal, and is held against the oracle's at the parity tolerance on every pixel; the light_space_shadows settings and
    coherent_waves = 0 are compared bit for bit under OFFSETS as well, border rays included."""
    A = T.lattice_answers(mesh, "near")
    cam = T.camera(T.NEAR)
    lower = T.lower_mesh(A["tris"], depth_of(mesh), eye=T.NEAR, floor=True)
    off_lines = np.array([(0.375, -0.125), (-0.125, 0.375), (0.125, 0.375), (-0.375, -0.125)])
    lower(oracle())
    want, _ = oracle().render(cam, W, Hh, 4, off_lines, tiles=T.TILES)
    frames, border = {}, {}
    twins = (("2", {}), ("1", {"light_space_shadows": 1}), ("0", {"light_space_shadows": 0}), ("per-lane", {"coherent_waves": 0}), ("edge_cull=0", {"edge_cull": 0}),
             ("primary_block_lists=0", {"primary_block_lists": 0}))
    for name, opts in twins:
        with options(hip, **opts):
            lower(hip)
            frames[name], _ = hip.render(cam, W, Hh, 4, off_lines, tiles=T.TILES)
            border[name], _ = hip.render(cam, W, Hh, len(T.OFFSETS), JITTER, tiles=T.TILES)
    for name, f in frames.items():
        assert np.array_equal(f, frames["2"]), f"light_space_shadows / coherent_waves twin {name} differs on {int(np.any(f != frames['2'], axis=2).sum())} pixels"
        assert np.array_equal(border[name], border["2"]), f"twin {name} differs on {int(np.any(border[name] != border['2'], axis=2).sum())} pixels of the border frame"
    worst = H.assert_frames_match(frames["2"], want, what=mesh_id(mesh))
    print(f"\n  {mesh_id(mesh)}: worst relative error against the oracle {worst:.2e}")
    assert worst < 1e-6
    lit = frames["2"][:32, :64].sum(axis=2)
    assert (lit > 0).sum() > 200 and (lit == 0).sum() > 50, "lit and shadowed pixels"


@gpu
@pytest.mark.parametrize("eye", list(EYES))
@pytest.mark.parametrize("mesh", LATTICE + GAPPED, ids=mesh_id)
def test_explicit_rays_equal_the_reference(hip, mesh, eye):
    """closest / blocked: mesh_bvh_query (bspMesh 0), mesh_bsp_query (depths 1 .. 3), the linear scan and the per-lane BSP walk of
    mesh_hits under CSG, the group of triangle primitives (the winner by its colour), and to_model under the exact transform."""
    A, scenes = lattice_scenes(mesh, eye)
    o, d, *_ = T.lattice_rays(eye)
    for name, (lower, by_colour) in scenes.items():
        lower(hip)
        check_rays(hip, A, o, d, f"{mesh_id(mesh)}/{eye}/{name}", winner=A["winner"] if by_colour else None, normals=depth_of(mesh) == 0 and mesh != "duplicates")


@gpu
@pytest.mark.parametrize("builder", [0, 1, 3])
def test_explicit_rays_under_every_bvh_builder(hip, builder):
    A = T.lattice_answers("sheet", "near")
    o, d, *_ = T.lattice_rays("near")
    with options(hip, bvh_builder=builder):
        T.lower_mesh(A["tris"], 0)(hip)
        check_rays(hip, A, o, d, f"sheet/bvh_builder={builder}", normals=True)


@gpu
@pytest.mark.parametrize("A", T.B_SIZES)
def test_band_on_explicit_rays(hip, A):
    cases, ref = band(A)
    for tri, rows in _by_triangle(cases, ref).items():
        check_small(hip, [tri], [(c[2], c[3], (r[0], r[1]), None) for c, r in rows], f"A={A!r}/{rows[0][0][0]}")


@gpu
@pytest.mark.parametrize("A", T.B_SIZES)
def test_subnormal_sh_on_explicit_rays(hip, A):
    """sh (or dq) stepped through the subnormals around 0.  On the ray o = (-5e-324, 0.25, 1) against A = 3 (and 3.900000000000001)
    sh = -5e-324 and a = A > 0, the reference's u = fl(fl(1 / A) * sh) is -0.0, which is not < 0.0, so Triangle.fs:54 goes on and the ray
    hits at t = 1.  A sign test `sh < 0 && a > 0` in front of the division rejects that ray (it did, on every path, until tri_hit took
    |sh| > |a| 2^-900 into the test: DESIGN.md 3 (iii), 15.5).  For A = 0.70000000000000417 and 1.7000000000000002 the product rounds to
    -5e-324 and the ray misses either way."""
    cases, ref = band(A, True)
    for tri, rows in _by_triangle(cases, ref).items():
        check_small(hip, [tri], [(c[2], c[3], (r[0], r[1]), None) for c, r in rows], f"A={A!r}/{rows[0][0][0]}")


@gpu
@pytest.mark.parametrize("A", T.B_SIZES)
def test_subnormal_sh_through_a_frames_wave(hip, A):
    """The same steps through tri_hit_wave (k_aov): at the eye (-5e-324, 0.25, 1) the reference hits triangle 0 at t = 1 for A = 3 and
    3.900000000000001 (see test_subnormal_sh_on_explicit_rays)."""
    cases, _ = band(A, True)
    groups = {}
    for c in cases:
        if c[3] == (0.0, 0.0, -1.0):
            groups.setdefault(c[1], []).append(c[2])
    for tri, eyes in groups.items():
        check_axial(hip, [tri], eyes, f"A={A!r}/subnormal")


@gpu
def test_epsilon_cases_on_explicit_rays(hip):
    for tri, rows in eps_rows().items():
        check_small(hip, [tri], [r[:4] for r in rows], rows[0][4])
    check_small(hip, T.DEGENERATE, degenerate_rows(), "degenerate")


# ---- the band and the epsilon cases through a frame's wave: the one pixel whose ray is (0, 0, -1)
AXIAL = (15, 31, (0.5, -0.5), [(8, 24, 8, 8)])                       # pixel, offset, its 8x8 tile
Z_EYE = 1.0
Z_START = Z_EYE - T.SLIGHT                                             # where the traced ray starts: one rounding, fused or not (0.0001 * -1 is exact)
Z_TRI = Z_START - 1.0                                                  # exact (Sterbenz): s_z = Z_START - Z_TRI == 1


def axial_triangles(tris):
    """The triangles moved to z = Z_TRI, and the filler that brings the mesh up to a tree."""
    moved = [tuple((p[0], p[1], p[2] + Z_TRI) for p in tri) for tri in tris]
    return T.with_filler(moved)


def axial_reference(tris, o):
    """The reference on the ray the device traces from an eye at (o.x, o.y, Z_EYE) through the axial pixel."""
    assert Z_START - Z_TRI == 1.0 and T.F(Z_START) - T.F(Z_TRI) == 1
    start, d = (o[0], o[1], Z_START), (0.0, 0.0, -1.0)
    best = (False, np.inf, -1)
    for i, tri in enumerate(tris):
        moved = tuple((p[0], p[1], p[2] + Z_TRI) for p in tri)
        assert T.exact_guard(moved, start, d)
        hit, t, _, _ = T.tri_reference(moved, start, d)
        if hit and t < best[1]:
            best = (True, t, i)
    return best


def axial_expectations(tris, eyes, depth):
    """(hit, t, triangle or None) per eye.  Depth 0: the reference.  Depth 1 (`bspMesh 1` of the triangles and the filler, which the cut
    at the middle of x separates without clipping): the branch box stands in front of the triangle test, and the axial ray runs along
    its faces with two zero direction components (0 * inf in BoundingBox.fs:32-58), so the box decides some eyes: the expectation is the
    oracle's closest hit of the ray the device traces, and the triangle is not named."""
    ref = [axial_reference(tris, o) for o in eyes]
    if depth == 0:
        return ref
    T.lower_mesh(axial_triangles(tris), depth)(oracle())
    start = np.array([(o[0], o[1], Z_START) for o in eyes])
    hit, t, _, _, _ = oracle().closest(start, np.broadcast_to(np.array([0.0, 0.0, -1.0]), start.shape).copy())
    return [(bool(h), float(tt) if h else np.inf, None) for h, tt in zip(hit, t)]


def check_axial(ctx, tris, eyes, what, depths=(0, 1)):
    """Per eye: render_aov's t and triangle at the axial pixel (k_aov), and a frame of that one pixel whose hits_primary is the
    expectation's hit (k_primary_mesh at depth 0, k_primary over the BSP at depth 1)."""
    x, y, off, tiles = AXIAL
    for depth in depths:
        want = axial_expectations(tris, eyes, depth)
        T.lower_mesh(axial_triangles(tris), depth)(ctx)
        for o, (hit, t, tri) in zip(eyes, want):
            cam = T.camera((o[0], o[1], Z_EYE))
            got = ctx.render_aov(cam, W, Hh, 1, np.array([off]), tiles=tiles, channels=["t", "triangle"])
            assert (got["triangle"][y, x] >= 0) == hit, f"{what}, depth {depth}, eye {o!r}: triangle {got['triangle'][y, x]}, expected {'a hit' if hit else 'a miss'}"
            assert tri is None or got["triangle"][y, x] == tri, f"{what}, depth {depth}, eye {o!r}: triangle {got['triangle'][y, x]}, the reference {tri}"
            assert got["t"][y, x] == t, f"{what}, depth {depth}, eye {o!r}: t {got['t'][y, x]!r}, expected {t!r}"
            _, st = ctx.render(cam, W, Hh, 1, np.array([off]), tiles=[(x, y, 1, 1)])
            assert st["hits_primary"] == int(hit), f"{what}, depth {depth}, eye {o!r}: the frame counts {st['hits_primary']} primary hits, expected {int(hit)}"


def test_axial_bsp_is_unclipped_and_the_oracle_agrees_with_the_reference_off_the_box_faces():
    """The depth-1 twin of the axial scenes: two leaves, the records the input's bit for bit; and how far the box decides - on the u = 1
    band of A = 3 the oracle at depth 1 equals the reference on every eye but those the box's face turns away (counted, printed)."""
    tri = T.band_triangle(3.0, 1.0, 0, False)
    ctx = ft.Context(host_only=True)
    try:
        tris = axial_triangles([tri])
        T.lower_mesh(tris, 1)(ctx)
        M = ctx.mesh_trees()
        t3 = tris.reshape(-1, 3, 3)
        want = np.concatenate([t3[:, 0], t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0]], axis=1)
        assert int(M["meshes"][0][0]) >= 0 and len(M["bsp_leaves"]) == 2 and M["tris"].shape[0] == len(t3) and np.array_equal(M["tris"], want[M["tri_src"]])
    finally:
        ctx.close()
    eyes = [c[2] for c in band(3.0)[0] if c[1] == tri and c[3] == (0.0, 0.0, -1.0)]
    ref, orc = axial_expectations([tri], eyes, 0), axial_expectations([tri], eyes, 1)
    same = sum(r[:2] == o[:2] for r, o in zip(ref, orc))
    print(f"\n  depth 1, A = 3: the oracle equals the reference on {same} of {len(eyes)} eyes; hits {sum(o[0] for o in orc)} (reference {sum(r[0] for r in ref)})")
    assert same >= len(eyes) // 2 and any(o[0] for o in orc) and not all(o[0] for o in orc)


def test_axial_rays_are_guarded_and_show_both_outcomes():
    for A in T.B_SIZES:
        rows = [c for c in band(A)[0] + band(A, True)[0] if c[3] == (0.0, 0.0, -1.0)]
        out = [axial_reference([c[1]], c[2])[0] for c in rows]
        assert len(rows) == 528 and 100 < sum(out) < 428
    assert T.pixel_dir(AXIAL[0], AXIAL[1], *AXIAL[2]) == (0, 0, -1)


@gpu
@pytest.mark.parametrize("coherent", [1, 0])
@pytest.mark.parametrize("A", T.B_SIZES)
def test_band_through_a_frames_wave(hip, A, coherent):
    """tri_hit_wave under mesh_bvh_packet (depth 0) and under mesh_bsp_packet / mesh_bsp_narrow (depth 1: a wave with zero direction
    components), in k_aov and in a frame's k_primary_mesh / k_primary, on sh = a (1 + k eps): the eye is stepped double by double."""
    cases, _ = band(A)
    groups = {}
    for c in cases:
        if c[3] == (0.0, 0.0, -1.0) and (coherent or c[0].startswith("one")):
            groups.setdefault(c[1], []).append(c[2])
    with options(hip, coherent_waves=coherent):
        for tri, eyes in groups.items():
            check_axial(hip, [tri], eyes, f"A={A!r}/coherent_waves={coherent}")


@gpu
def test_epsilon_cases_through_a_frames_wave(hip):
    groups = {}
    for label, tri, o, d, _ in T.eps_cases():
        if d == (0.0, 0.0, -1.0) and o[2] == 1.0:
            groups.setdefault(tri, []).append(o)
    assert len(groups) >= 7
    for tri, eyes in groups.items():
        check_axial(hip, [tri], eyes, "epsilon")
    check_axial(hip, T.DEGENERATE, [r[0] for r in degenerate_rows()], "degenerate")

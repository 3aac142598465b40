"""Scenes far from the origin and at extreme scales, against the CPU oracle.

The hot path is FP64, but many float32 tests in front of it throw work away when it "certainly" cannot produce a hit.  The
rounding of a float coordinate grows with its magnitude, not with the distances being compared, so a cull whose slack has
no magnitude term passes every unit-scale test and silently drops hits once a scene sits far from the origin.  Every
scene here keeps the item structure of its unshifted self, and the rays are aimed to hit within 1e-3 .. 0.05 of the points
farthest from an item's bounding-sphere centre: there the FP64 hit / miss decision is well conditioned (the rounding at
1e6 is ~1e-10), so only a cull can make the device and the oracle disagree."""
import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from .test_gpu_fuzz import SceneRecipe
from .test_light_space_grid import render_three
from .test_light_space_shadows import bunny_tris

OFFSETS = [0.0, 1e3, 1e4, 1e5, 1e6]
SCENES = list(H.PRIMS) + ["csg", "mesh0", "mesh12", "mesh_translated"]
STRUCTURE = ("items", "bounded_items", "face_directions")


def offset_vectors(T):
    """The offset with mixed signs per axis, and the same plus half a float ulp of T (the float rounding of a centre there is
    as large as it can be: exactly half an ulp)."""
    if T == 0.0:
        return [np.zeros(3)]
    half = 0.5 * float(np.spacing(np.float32(T)))
    return [T * np.array([1.0, -1.0, 1.0]), (T + half) * np.array([-1.0, 1.0, 1.0])]


def small_mesh():
    """The headline's stand-in mesh at about unit size, near the origin."""
    return bunny_tris() * 4.0


# ---- the scenes: a target item at T and two more top-level items beside it (three items: the item mask is in play) ----------

MODEL_BOX = {"sphere": ((-1, -1, -1), (1, 1, 1)), "cube": ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), "square": ((0, 0, 0), (1, 0, 1)),
             "circle": ((-1, 0, -1), (1, 0, 1)), "cone": ((-1, 0, -1), (1, 1, 1)), "cylinder": ((-1, 0, -1), (1, 1, 1)),
             "solidCylinder": ((-1, 0, -1), (1, 1, 1)), "plane": ((-2, 0, -2), (2, 0, 2)), "csg": ((-1, -1, -1), (1, 1, 2))}
SPHERE_AT, CUBE_AT = np.array([2.6, 0.3, 0.0]), np.array([-2.2, 0.0, 0.7])


def target_node(b, kind, T):
    """The scene's first item, positioned at T: (node, its world-space mesh triangles or None)."""
    if kind == "csg":
        return b.translate(tuple(T), b.union(b.primitive(ft.SPHERE), b.translate((0, 0, 1), b.primitive(ft.SPHERE)))), None
    if kind.startswith("mesh"):
        tris = small_mesh()
        if kind == "mesh_translated":
            return b.translate(tuple(T), b.bsp_mesh(0, tris)), tris + np.tile(T, 3)
        world = tris + np.tile(T, 3)                                          # a bare mesh: the vertices themselves sit at the offset
        return b.bsp_mesh(0 if kind == "mesh0" else 12, world), world
    return b.translate(tuple(T), b.primitive(H.PRIMS[kind])), None


def offset_scene(b, kind, T):
    b.clear()
    T = np.asarray(T, dtype=np.float64)
    node, tris = target_node(b, kind, T)
    items = [b.material(node, colour=(0.9, 0.6, 0.3), reflectance=0.3, shineyness=5.0),
             b.material(b.translate(tuple(T + SPHERE_AT), b.primitive(ft.SPHERE)), colour=(0.3, 0.8, 0.4)),
             b.material(b.translate(tuple(T + CUBE_AT), b.primitive(ft.CUBE)), colour=(0.5, 0.5, 0.9), reflectance=0.5)]
    b.set_objects(b.group(items))
    b.add_directional((0.3, -1.0, 0.5), (1, 1, 1))
    b.add_positional(tuple(T + (1.0, 5.0, -2.0)), (1.0, 0.01, 0.02), (0.6, 0.6, 0.6))
    b.commit()
    return tris


# ---- surface points near the extremes of each item, with their normals (model space) --------------------------------------------

def surface_points(kind, rng, delta):
    k = delta.size
    a = rng.uniform(0, 2 * np.pi, k)
    c, s = np.cos(a), np.sin(a)
    sg = lambda: rng.choice([-1.0, 1.0], k)
    zero, one = np.zeros(k), np.ones(k)
    if kind in ("sphere", "plane"):
        if kind == "plane":
            return np.stack([rng.uniform(-2, 2, k), zero, rng.uniform(-2, 2, k)], 1), np.stack([zero, one, zero], 1)
        u = rng.normal(size=(k, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        return u, u
    if kind == "cube":                                                    # on a face, within delta of the face's corner
        axis = rng.integers(0, 3, k)
        p = np.stack([sg(), sg(), sg()], 1) * (0.5 - delta[:, None] * rng.uniform(1.0, 2.0, (k, 3)))
        side = sg()
        p[np.arange(k), axis] = 0.5 * side
        n = np.zeros((k, 3)); n[np.arange(k), axis] = side
        return p, n
    if kind == "square":
        pick = lambda: np.where(rng.random(k) < 0.5, delta * rng.uniform(1.0, 2.0, k), 1.0 - delta * rng.uniform(1.0, 2.0, k))
        return np.stack([pick(), zero, pick()], 1), np.stack([zero, one, zero], 1)
    if kind == "circle":
        return np.stack([(1 - delta) * c, zero, (1 - delta) * s], 1), np.stack([zero, one, zero], 1)
    if kind == "cone":                                                    # apex at y = 1, open base rim of radius 1 at y = 0
        return np.stack([(1 - delta) * c, delta, (1 - delta) * s], 1), np.stack([c, one, s], 1) / np.sqrt(2.0)
    if kind in ("cylinder", "solidCylinder"):
        y = np.where(rng.random(k) < 0.5, delta, 1.0 - delta)
        p, n = np.stack([c, y, s], 1), np.stack([c, zero, s], 1)
        if kind == "solidCylinder":                                       # half of them on the caps, near the rim
            cap = rng.random(k) < 0.5
            capy = np.where(rng.random(k) < 0.5, 0.0, 1.0)
            p[cap] = np.stack([(1 - delta) * c, capy, (1 - delta) * s], 1)[cap]
            n[cap] = np.stack([zero, 2 * capy - 1, zero], 1)[cap]
        return p, n
    if kind == "csg":                                                     # union of the spheres at z = 0 and z = 1: the far caps
        u = rng.normal(size=(k, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        u[:, 2] = np.abs(u[:, 2]) * sg()
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        far = np.abs(u[:, 2]) > 0.3
        u = u[far]
        return u + np.where(u[:, 2:3] > 0, 1.0, 0.0) * np.array([0, 0, 1.0]), u
    raise KeyError(kind)


def mesh_points(tris, rng, delta):
    """Points on the triangles around the vertices farthest from the mesh's box centre, delta in from the vertex."""
    v = tris.reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    d2 = np.sum((v - 0.5 * (lo + hi)) ** 2, axis=2)
    far = np.argsort(d2.max(axis=1))[::-1][:16]                          # the triangles holding the farthest vertices
    t = far[rng.integers(0, far.size, delta.size)]
    corner = v[t, np.argmax(d2[t], axis=1)]
    cen = v[t].mean(axis=1)
    step = np.minimum(delta, 0.5 * np.linalg.norm(cen - corner, axis=1))
    p = corner + (cen - corner) * (step / np.linalg.norm(cen - corner, axis=1))[:, None]
    n = np.cross(v[t, 1] - v[t, 0], v[t, 2] - v[t, 0])
    return p, n / np.linalg.norm(n, axis=1, keepdims=True)


def rays_through(p, n, centre, rng, back=3.0):
    """Rays that cross the surface at p (transversally: |cos| >= 0.2 with the normal), half of them tangent to the sphere about
    `centre` through p (the rays the bounding-sphere test judges most closely), the rest from random directions.  Directions are
    not normalised (Image.fs:88-89)."""
    k = p.shape[0]
    d = rng.normal(size=(k, 3))
    radial = p - centre
    radial /= np.maximum(np.linalg.norm(radial, axis=1, keepdims=True), 1e-300)
    tangent = rng.random(k) < 0.5
    d[tangent] -= np.sum(d[tangent] * radial[tangent], axis=1, keepdims=True) * radial[tangent]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    keep = np.abs(np.sum(d * n, axis=1)) >= 0.2
    p, d = p[keep], d[keep]
    o = p - back * d
    return o, d * rng.uniform(0.2, 3.0, size=(p.shape[0], 1))


def log_deltas(rng, k):
    return np.exp(rng.uniform(np.log(1e-3), np.log(0.05), k))


def one_per_wave(o, d, T, seed):
    """Each ray in a wave of its own, beside 63 rays that start above the scene and climb away from it.  A wave-level cull keeps an
    item when any lane may hit it, so a ray it wrongly turns away only loses its hit when no other lane of its wave needs that item:
    alone among rays that certainly miss everything, every aimed ray is judged on its own."""
    rng = np.random.default_rng(seed)
    n = o.shape[0]
    fo = np.asarray(T, dtype=np.float64) + np.array([0.0, 40.0, 0.0]) + rng.uniform(-3, 3, size=(n, 63, 3))
    fd = np.concatenate([rng.uniform(-0.2, 0.2, size=(n, 63, 1)), np.ones((n, 63, 1)), rng.uniform(-0.2, 0.2, size=(n, 63, 1))], axis=2)
    return (np.concatenate([o[:, None, :], fo], axis=1).reshape(-1, 3), np.concatenate([d[:, None, :], fd], axis=1).reshape(-1, 3))


def aimed_rays(kind, T, tris, seed, n=1500):
    """Rays at the target item's extremes and the cube item's corners, each alone in its wave, then random rays around the offset."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, dtype=np.float64)
    if tris is not None:
        p, nr = mesh_points(tris, rng, log_deltas(rng, n))
        v = tris.reshape(-1, 3)
        centre = 0.5 * (v.min(0) + v.max(0))
    else:
        p, nr = surface_points(kind, rng, log_deltas(rng, n))
        lo, hi = (np.asarray(x, dtype=np.float64) for x in MODEL_BOX[kind])
        centre = T + 0.5 * (lo + hi)
        p = p + T
    o1, d1 = rays_through(p, nr, centre, rng)
    pc, nc = surface_points("cube", rng, log_deltas(rng, n // 3))
    o2, d2 = rays_through(pc + T + CUBE_AT, nc, T + CUBE_AT, rng)
    o3, d3 = H.random_rays(512, seed=seed, origin_scale=3.0, toward=(0, 0, 0), spread=1.5)
    o, d = one_per_wave(np.concatenate([o1, o2]), np.concatenate([d1, d2]), T, seed)
    return np.concatenate([o, o3 + T]), np.concatenate([d, d3])


def assert_rays_match(hip, orc, o, d, what, max_depth=8, seed=0):
    H.assert_hits_match(hip.closest(o, d), orc.closest(o, d), what=what)
    md = np.abs(np.random.default_rng(seed).normal(size=o.shape[0])) * 4.0 / np.linalg.norm(d, axis=1)
    assert np.array_equal(hip.blocked(o, d, md), orc.blocked(o, d, md)), f"{what}: lightIsBlocked differs"
    got, want = hip.colour_for_ray(o, d, max_depth=max_depth), orc.colour_for_ray(o, d, max_depth=max_depth)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN colours differ"
    H.assert_frames_match(np.where(nan, 0.0, got)[:, None, :], np.where(nan, 0.0, want)[:, None, :], what=what)


def structure(ctx):
    info = ctx.scene_info()
    return {k: info[k] for k in STRUCTURE}


# ---- the shifted / scaled random scenes and the headline mesh ------------------------------------------------------------------

FUZZ_SHIFTS = [(1e4, 1001), (1e4, 1005), (1e4, 1012), (1e5, 1001), (1e5, 1007), (1e5, 1020), (1e6, 1003), (1e6, 1005), (1e6, 1012)]
FUZZ_SCALES = [(1e-3, 1001), (1e-3, 1009), (1e3, 1001), (1e3, 1009)]
FUZZ_OFFSET_DIR = np.array([1.0, -1.0, 1.0])
EYE, LOOK_AT = np.array([1.0, 2.0, -9.0]), np.zeros(3)


def fuzz_map(T, s):
    off = T * FUZZ_OFFSET_DIR
    return off, s, lambda x: s * np.asarray(x, dtype=np.float64) + off


BUNNY_OFFSET = 1e5 * np.array([1.0, 1.0, -1.0])


def bunny_world():
    """scenes/bunny.scene's mesh with its transform (scale 8, rotate 180 degrees about y) applied to the vertices."""
    v = bunny_tris().reshape(-1, 3) * 8.0
    v[:, 0], v[:, 2] = -v[:, 0], -v[:, 2]
    return v.reshape(-1, 9)


def bunny_scene(depth, T):
    tris = bunny_world() + np.tile(T, 3)
    floor_y = float(tris.reshape(-1, 3)[:, 1].min())

    def lower(b):
        b.clear()
        items = [b.material(b.bsp_mesh(depth, tris), colour=(1, 1, 1)),
                 b.material(b.translate((T[0], floor_y, T[2]), b.primitive(ft.PLANE)), colour=(0.6, 0.6, 0.6), reflectance=0.5),
                 b.material(b.translate(tuple(T + (-1.5, 0.8, 3.0)), b.primitive(ft.SPHERE)), colour=(0.8, 0.3, 0.3), reflectance=0.4)]
        b.set_objects(b.group(items))
        b.add_directional((-3, -2, 3), (1, 1, 1))
        b.commit()
    cam = ft.make_camera(tuple(T + (0.0, 2.0, -2.0)), tuple(T + (0.0, 0.0, 3.0)), (0, 1, 0), H.deg(60.0), 1.0)
    return lower, cam


# ---- CPU: the shifted scenes keep their structure, and the oracle is well conditioned there ------------------------------------

def test_shifted_and_scaled_scenes_keep_their_item_structure():
    ctx = ft.Context(host_only=True)
    try:
        for kind in SCENES:
            offset_scene(ctx, kind, np.zeros(3))
            want = structure(ctx)
            assert want["items"] >= 3
            for T in OFFSETS[1:]:
                for Tv in offset_vectors(T):
                    offset_scene(ctx, kind, Tv)
                    assert structure(ctx) == want, f"{kind} at {Tv}"
        for seed in sorted({s for _, s in FUZZ_SHIFTS + FUZZ_SCALES}):
            recipe = SceneRecipe(seed)
            recipe.build(ctx)
            want = structure(ctx)
            for T, s in [(T, 1.0) for T, k in FUZZ_SHIFTS if k == seed] + [(0.0, s) for s, k in FUZZ_SCALES if k == seed]:
                off, sc, _ = fuzz_map(T, s)
                recipe.build(ctx, offset=off, scale=sc)
                assert structure(ctx) == want, f"recipe {seed} at T={T}, s={s}"
        for depth in (0, 12):
            lower, _ = bunny_scene(depth, np.zeros(3))
            lower(ctx)
            want = structure(ctx)
            lower, _ = bunny_scene(depth, BUNNY_OFFSET)
            lower(ctx)
            assert structure(ctx) == want, f"bunny depth {depth}"
    finally:
        ctx.close()


def test_recipe_offset_of_nothing_draws_the_same_scene():
    """The offset / scale arguments leave a recipe's own draws alone: seeds keep drawing the scenes the fuzz suite knows."""
    a, b = SceneRecipe(1001), SceneRecipe(1001)
    assert a.calls == b.calls
    orc = O.Oracle()
    o, d = H.random_rays(500, seed=3, origin_scale=4.0, toward=(0, 0, 0), spread=3.0)
    a.build(orc)
    plain = orc.closest(o, d)
    a.build(orc, offset=(0.0, 0.0, 0.0), scale=1.0)                     # the identity, spelled out: wraps each item in a transform
    H.assert_hits_match(orc.closest(o, d), plain, what="identity offset")


T_FAR = np.array([1e6, -1e6, 1e6])


def test_oracle_cube_corner_hit_at_1e6_is_analytic():
    orc = O.Oracle()
    orc.clear()
    orc.set_objects(orc.group([orc.translate(tuple(T_FAR), orc.primitive(ft.CUBE))]))
    orc.commit()
    o = T_FAR + (2.5, 0.35, -0.4)
    d = np.array([-2.0, 0.1, -0.05])                                      # reaches x = T + 0.5 at t = 1, 0.05 in from the corner
    hit, t, p, n, _ = orc.closest([o], [d])
    assert hit[0]
    assert abs(t[0] - 1.0) <= 1e-9
    assert np.allclose(p[0], T_FAR + (0.5, 0.45, -0.45), rtol=0, atol=1e-9)
    assert np.allclose(n[0], (1.0, 0.0, 0.0), rtol=0, atol=1e-9)


def test_oracle_sphere_hit_at_1e6_is_analytic():
    orc = O.Oracle()
    orc.clear()
    orc.set_objects(orc.group([orc.translate(tuple(T_FAR), orc.primitive(ft.SPHERE))]))
    orc.commit()
    o = T_FAR + (0.6, 0.0, -5.0)
    d = np.array([0.0, 0.0, 2.0])                                         # meets x^2 + z^2 = 1 at z = -0.8: t = 4.2 / 2
    hit, t, p, n, _ = orc.closest([o], [d])
    assert hit[0]
    assert abs(t[0] - 2.1) <= 1e-9
    assert np.allclose(p[0], T_FAR + (0.6, 0.0, -0.8), rtol=0, atol=1e-9)
    assert np.allclose(n[0], (0.6, 0.0, -0.8), rtol=0, atol=1e-9)


# ---- on the device -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T", OFFSETS)
@pytest.mark.parametrize("kind", SCENES)
def test_rays_at_item_extremes_match_oracle(hip, kind, T):
    orc = O.Oracle()
    offset_scene(hip, kind, np.zeros(3))
    want_structure = structure(hip)
    for j, Tv in enumerate(offset_vectors(T)):
        tris = offset_scene(hip, kind, Tv)
        offset_scene(orc, kind, Tv)
        assert structure(hip) == want_structure
        o, d = aimed_rays(kind, Tv, tris, seed=17 * j + 3)
        assert_rays_match(hip, orc, o, d, what=f"{kind} at {Tv.tolist()}", seed=j)


@pytest.mark.gpu
@pytest.mark.parametrize("mag", [1e-16, 1e-8, 1e-3, 1e3, 1e8, 1e16])
@pytest.mark.parametrize("T", [0.0, 1e5, 1e6])
def test_extreme_direction_magnitudes_match_oracle(hip, T, mag):
    """The reference does not normalise directions: the float pre-test normalises them itself, and beyond its window (|d|^2
    outside 1e-30 .. 1e30) gives no verdict at all."""
    orc = O.Oracle()
    Tv = offset_vectors(T)[-1]
    for b in (hip, orc):
        offset_scene(b, "cube", Tv)
    o, d = aimed_rays("cube", Tv, None, seed=int(np.log10(mag)) + 40)
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * mag
    assert_rays_match(hip, orc, o, d, what=f"|d| = {mag} at {Tv.tolist()}")


def _check_recipe_frames(hip, seed, T, s, extra_frames):
    off, sc, at = fuzz_map(T, s)
    recipe = SceneRecipe(seed)
    orc = O.Oracle()
    recipe.build(hip)
    want_structure = structure(hip)
    recipe.build(orc, offset=off, scale=sc)
    recipe.build(hip, offset=off, scale=sc)
    assert structure(hip) == want_structure
    what = f"recipe {seed} at T={T}, s={s}"
    o, d = H.random_rays(2000, seed=seed, origin_scale=4.0, toward=(0, 0, 0), spread=3.0)
    H.assert_hits_match(hip.closest(at(o), d), orc.closest(at(o), d), what=what)
    cam = ft.make_camera(tuple(at(EYE)), tuple(at(LOOK_AT)), (0, 1, 0), H.deg(55.0))
    frames = [("frame", 96, 64, 2)]
    if extra_frames:
        frames += [("depth of field", 48, 32, 2), ("corner sampling", 40, 24, 0)]
    for name, w, h, spp in frames:
        cam.has_focus, cam.focal_length, cam.aperture_angular_size = (1, 9.0 * s, 0.02) if name == "depth of field" else (0, 0.0, 0.0)
        jit = ft.jitter_pattern(spp) if spp else None
        want, ost = orc.render(cam, w, h, spp, jit, seed=ft.DEFAULT_SEED)
        got, st = hip.render(cam, w, h, spp, jit, seed=ft.DEFAULT_SEED)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what} {name}: NaN pixels differ"
        assert H.assert_frames_match(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what=f"{what} {name}") < 1e-6
        assert st["rays_reference_equivalent"] == ost["rays_traced"]


@pytest.mark.gpu
@pytest.mark.parametrize("T,seed", FUZZ_SHIFTS)
def test_shifted_random_scene_matches_oracle(hip, T, seed):
    hip.set_option("csg_mesh_capacity", 16)
    try:
        _check_recipe_frames(hip, seed, T, 1.0, extra_frames=seed == 1001)
    finally:
        hip.set_option("csg_mesh_capacity", 32)


@pytest.mark.gpu
@pytest.mark.parametrize("s,seed", FUZZ_SCALES)
def test_scaled_random_scene_matches_oracle(hip, s, seed):
    """slightOffset and the shadow-ray offset are absolute (Shading.fs:109-117, 129): a scaled frame is not the unscaled one
    scaled, so the judge is the oracle, not invariance."""
    hip.set_option("csg_mesh_capacity", 16)
    try:
        _check_recipe_frames(hip, seed, 0.0, s, extra_frames=seed == 1001)
    finally:
        hip.set_option("csg_mesh_capacity", 32)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,builder", [(0, 1), (0, 0), (12, 0)])
def test_headline_mesh_far_from_origin(hip, depth, builder):
    """The headline mesh with its vertices 1e5 out, over a reflective floor (the bounces take the incoherent path): BVH / tree /
    grid shadows give the same bits, and a reduced frame matches the oracle."""
    lower, cam = bunny_scene(depth, BUNNY_OFFSET)
    hip.set_option("bvh_builder", builder)
    try:
        render_three(hip, lower, cam, 160, 160, 2)
        if depth == 0:
            assert (hip.commit_times()["device_bvh_height"] > 0) == (builder == 1)
        orc = O.Oracle()
        lower(orc)
        lower(hip)                                                          # (render_three's last option change asks for a new commit)
        jit = ft.jitter_pattern(1)
        want, ost = orc.render(cam, 48, 48, 1, jit, seed=ft.DEFAULT_SEED)
        got, st = hip.render(cam, 48, 48, 1, jit, seed=ft.DEFAULT_SEED)
        assert H.assert_frames_match(got, want, what=f"bunny at 1e5, depth {depth}, builder {builder}") < 1e-6
        assert st["rays_reference_equivalent"] == ost["rays_traced"]
    finally:
        hip.set_option("bvh_builder", 2)

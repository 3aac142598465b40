"""The device path at its documented limits, and one past each.

A lane's state is packed into fixed bytes and slots: sixteen 8-bit list marks in two registers (CSG nesting <= 8, <= 255 hits per ray in
a CSG subtree), one occluded-sample byte per light in two registers (<= 16 lights, <= 255 soft samples), one cursor and one ray count
per reflection level (max_depth <= 16).  The scenes here fill those bytes and slots to the last one - 16 live marks, a list and a mark of
255, light 15 fully occluded at 255 samples beside its neighbours, level 16 alive - and compare with the CPU oracle, which recurses
over std::vector and has none of these limits (oracle/ft_oracle.cpp: the hit lists are vectors, Csg nests by recursion, the lights are a
vector looped over, the samples a loop count, the recursion limit an int), and with closed forms that involve no tracer at all.
One past each limit the commit (or the frame) is refused with its own message, and what was committed before stays renderable.

The first half runs without a GPU: host-only contexts, the oracle, numpy.  The scenes are built in tests/limit_tools.py."""
import functools

import numpy as np
import pytest

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import helpers as H
from . import limit_tools as T
from .test_light_space_grid import render_three

gpu = pytest.mark.gpu
CSG_NAMES = list(T.csg_cases())
JIT2 = ft.jitter_pattern(2)


def _cam(spec, aspect=64 / 48):
    return ft.make_camera(spec[0], spec[1], spec[2], H.deg(spec[3]), aspect)


def _frames_match(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pixels differ"
    assert not np.isnan(want).any(), f"{what}: the scene is meant to have no NaN pixel"
    assert H.assert_frames_match(got, want, what=what) < 1e-6


def _refused(call, *words):
    """`call` must fail with FT_ERR_UNSUPPORTED and a message holding every one of `words`."""
    with pytest.raises(ft.FtError) as e:
        call()
    assert e.value.status == -4, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


# =============================================================================================================================
# References, computed once per session on the oracle and shared by the CPU and the GPU half.

@functools.lru_cache(maxsize=None)
def csg_reference(name):
    orc = O.Oracle()
    T.build_csg_case(orc, name)
    o, d = T.csg_rays(seed=CSG_NAMES.index(name))
    md = np.abs(np.random.default_rng(50 + CSG_NAMES.index(name)).normal(size=o.shape[0])) * 6.0
    frame, stats = orc.render(_cam(T.CSG_CAMERA), 64, 48, 2, JIT2)
    return {"orc": orc, "o": o, "d": d, "md": md, "closest": orc.closest(o, d), "blocked": orc.blocked(o, d, md), "frame": frame, "stats": stats}


@functools.lru_cache(maxsize=None)
def stack_reference():
    orc = O.Oracle()
    T.build_stack(orc)
    o, d = T.stack_rays(STACK_KS)
    o2, d2 = H.random_rays(1500, seed=21, origin_scale=4.0, toward=(120.0, 0.5, 12.0), spread=60.0)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    md = np.concatenate([np.full(len(STACK_KS) + 4, 1e9), np.abs(np.random.default_rng(22).normal(size=1500)) * 40.0])
    frame, stats = orc.render(_cam(STACK_CAMERA, 32 / 24), 32, 24, 1, ft.jitter_pattern(1))
    return {"o": o, "d": d, "md": md, "closest": orc.closest(o, d), "blocked": orc.blocked(o, d, md), "all": orc.all_hits(o[:len(STACK_KS) + 4], d[:len(STACK_KS) + 4], cap=300),
            "frame": frame, "stats": stats}


@functools.lru_cache(maxsize=None)
def mirror_reference(fancy):
    orc = O.Oracle()
    T.build_mirror_hall(orc, fancy)
    o, d = T.mirror_rays()
    out = {"o": o, "d": d}
    for depth in T.DEPTHS:
        frame, stats = orc.render(_cam(T.MIRROR_CAMERA, 48 / 32), 48, 32, 1, ft.jitter_pattern(1), max_depth=depth)
        out[depth] = {"rays": orc.colour_for_ray(o, d, max_depth=depth), "frame": frame, "stats": stats}
    return out


STACK_KS = (1, 127, 128, 200, 250, T.STACK_N)                     # the last: every triangle, the largest count the scene allows
STACK_CAMERA = ((60.0, 30.0, -70.0), (100.0, 0.5, 12.0), (0, 1, 0), 60.0)


# =============================================================================================================================
# CPU half

def test_csg_cases_hold_the_marks_they_claim():
    """By construction (limit_tools.tree_facts, which mirrors Flattener::walk's OP_MARK / OP_CSG_PAIR rules), not by measurement: the
    right-deep chains of depth 5 .. 8 hold 10 .. 16 marks because their innermost B operand is not a bare primitive - a Group of two
    primitives (x_group), a Group of bare triangles (x_tris) or a bspMesh (x_mesh): bare_primitive() in ft_scene.cpp follows
    Transform / Material / HueShift / IgnoreLight / Texture nodes down to a Prim and answers false for anything else, a Group or a
    Mesh included, and a pair needs both operands bare.  The left-deep chain holds depth + 1; the chain that ends in a bare
    primitive fuses its last level and pushes that pair's hits under 14 marks, six of them in marks_hi."""
    facts = {name: T.tree_facts(tree) for name, (tree, _) in T.csg_cases().items()}
    for name, depth, marks in (("right5", 5, 10), ("right6", 6, 12), ("right7", 7, 14), ("right8", 8, 16), ("right8-shift0", 8, 16), ("right8-shift1", 8, 16),
                               ("right8-shift3", 8, 16), ("right8-transformed", 8, 16), ("right8-beside", 8, 16), ("left8", 8, 9), ("mixed8", 8, 16)):
        assert (facts[name]["depth"], facts[name]["marks"]) == (depth, marks), (name, facts[name])
        assert facts[name]["marks_under_pair"] < 9
    pairs = facts["right8-shift2-pairs"]
    assert pairs["depth"] == 8 and pairs["marks"] == 14 and pairs["marks_under_pair"] == 14      # OP_CSG_PAIR with in_csg under marks 9 .. 14
    assert facts["mixed8"]["marks_under_pair"] == 4
    covered = set().union(*(f["ops"] for f in facts.values()))
    assert covered == {(level, op) for level in range(1, 9) for op in T.OPS}, "all four operators at every level across the cases"
    assert sum(f["marks_at_skip"] >= 9 for f in facts.values()) >= 6, "OP_SKIP_IF_EMPTY under 9 or more marks"
    ctx = ft.Context(host_only=True)
    for name in CSG_NAMES:                                          # and the flattener takes every one of them
        T.build_csg_case(ctx, name)
        info = ctx.scene_info()
        assert info["items"] == (3 if name == "right8-beside" else 1) and 20 <= info["csg_capacity"] <= 80, (name, info)
    ctx.close()


@pytest.mark.parametrize("name", CSG_NAMES)
def test_csg_cases_are_alive_on_the_oracle(name):
    """On the oracle alone: at least a quarter of the rays hit, and at least a tenth of the hits carry a flipped normal or come from
    inside the B operand of a level below 4 (here: of level 5 or deeper) - a chain that carved everything away, or that shows the
    outermost operand only, would pass every comparison as an empty frame."""
    ref = csg_reference(name)
    plain = O.Oracle()
    T.build_csg_case(plain, name, no_csg=True)
    hit_share, alive_share = T.csg_liveness(ref["orc"], plain, name, ref["o"], ref["d"])
    assert hit_share >= 0.25 and alive_share >= 0.10, (name, hit_share, alive_share)
    assert (ref["frame"].sum(axis=2) > 0).mean() >= 0.1, "the frame shows the item"
    assert ref["closest"][0][4000:].sum() >= 100, "the axis-parallel rays hit too"


# The onion: concentric spheres S9 .. S1 (radius k about the origin), S9 op (S8 op (... (S2 op {S1}))), 16 marks.
#
# "alternate": subtract, union, subtract, ... from the outside in.  From the inside out: S2 + S1 is the ball of radius 2 (union drops
# S1's hits, both inside S2: BIntoAB, ABleaveB); S3 - ball is the shell 2 .. 3; S4 + shell is the ball of radius 4 again; ...; S8 + ...
# is the ball of radius 8 and the whole thing the shell 8 .. 9.  Its inner surface is S8's, flipped once by the outermost subtract.
#
# "subtract": all eight subtract.  X1 = S1, Xk = Sk - X(k-1): X2 = [1, 2], X3 = [0, 1] + [2, 3], ..., X9 = [0, 1] + [2, 3] + [4, 5] +
# [6, 7] + [8, 9] (ranges of the radius).  Every one of the nine spheres bounds the solid.  Sk (k >= 2) is the A operand of level 10 - k
# and lies inside the B operand of the 9 - k levels above it, each of which flips it (Csg.fs:36-44: subtract keeps B's hits inside A,
# flipped): Sk's normal is the outward one for odd k and the inward one for even k.  S1 is flipped by all 8 levels: outward.
ONION = {
    "alternate": ([ft.SUBTRACT, ft.UNION] * 4, [
        # origin, direction (not normalised), t, p, n
        ((0, 0, -20), (0, 0, 1), 11.0, (0, 0, -9), (0, 0, -1)),    # from outside: S9, outward
        ((0, 0, 0), (0, 0, 1), 8.0, (0, 0, 8), (0, 0, -1)),        # from the hollow: S8 at 8, flipped: toward the centre
        ((20, 0, 0), (-2, 0, 0), 5.5, (9, 0, 0), (1, 0, 0)),
        ((0, 8.5, 0), (0, 1, 0), 0.5, (0, 9, 0), (0, 1, 0)),       # from inside the shell outward: S9 from within, the outward normal as it is
        ((0, 8.5, 0), (0, -1, 0), 0.5, (0, 8, 0), (0, -1, 0))]),   # from inside the shell inward: S8, flipped
    "subtract": ([ft.SUBTRACT] * 8, [
        ((0, 0, 0), (0, 0, 1), 1.0, (0, 0, 1), (0, 0, 1)),         # inside the core: S1, 8 flips: outward
        ((0, 0, 1.5), (0, 0, 1), 0.5, (0, 0, 2), (0, 0, -1)),      # in the gap 1 .. 2: S2, 7 flips: inward
        ((0, 0, -20), (0, 0, 1), 11.0, (0, 0, -9), (0, 0, -1)),    # S9, no flip
        ((0, 5.5, 0), (0, 1, 0), 0.5, (0, 6, 0), (0, -1, 0)),      # in the gap 5 .. 6: S6, 3 flips: inward
        ((4.5, 0, 0), (1, 0, 0), 0.5, (5, 0, 0), (1, 0, 0)),       # in the solid 4 .. 5: S5, 4 flips: outward
        ((0, 0, 3.5), (0, 0, -0.5), 1.0, (0, 0, 3), (0, 0, 1)),    # in the gap 3 .. 4 looking in: S3, 6 flips: outward
        ((0, -7.25, 0), (0, -1, 0), 0.75, (0, -8, 0), (0, 1, 0))]),   # in the gap 7 .. 8: S8, 1 flip: toward the centre
}


def _check_onion(b, which):
    ops, rays = ONION[which]
    T.onion(b, ops)
    hit, t, p, n, _ = b.closest([r[0] for r in rays], [r[1] for r in rays])
    for k, (_, _, wt, wp, wn) in enumerate(rays):
        assert hit[k] == 1, (which, k)
        assert abs(t[k] - wt) <= 1e-12 * max(1.0, wt), (which, k, t[k], wt)
        assert np.allclose(p[k], wp, rtol=0, atol=1e-12) and np.allclose(n[k], wn, rtol=0, atol=1e-12), (which, k, p[k], n[k])


@pytest.mark.parametrize("which", list(ONION))
def test_onion_closed_form_on_the_oracle(which):
    _check_onion(O.Oracle(), which)
    ctx = ft.Context(host_only=True)
    T.onion(ctx, ONION[which][0])
    assert ctx.scene_info()["csg_capacity"] == 18                  # 9 spheres, 2 hits each
    ctx.close()


def _info_or_status(ctx):
    try:
        return ctx.scene_info()
    except ft.FtError as e:
        return e.status


def test_one_past_each_commit_limit_is_refused_with_its_own_message():
    """9 levels, 256 hits, 17 lights, a 256-sample light: FT_ERR_UNSUPPORTED, each with a message that names its limit, and the
    context answers for the commit it held before as if the refused one had not been tried."""
    ctx = ft.Context(host_only=True)
    H.single_prim(ctx, "sphere")
    before = ctx.scene_info()

    def nine_levels():
        ctx.clear()
        ctx.set_objects(ctx.group([T.build_tree(ctx, T.right_deep(9, 0, T.x_group))]))
        ctx.commit()

    def hits_256():
        ctx.set_option("csg_mesh_capacity", T.STACK_N + 1)
        T.build_stack(ctx, T.STACK_N + 1)

    for attempt, words in ((nine_levels, ("deeper than 8",)), (hits_256, ("255 hits",)), (lambda: T.build_lights_scene(ctx, n_lights=17), ("16 lights",)),
                           (lambda: T.build_lights_scene(ctx, soft=(15,), samples=256), ("255 samples",))):
        try:
            _refused(attempt, *words)
            assert ctx.scene_info() == before
        finally:
            ctx.set_option("csg_mesh_capacity", 32)                 # (a commit-time option: the next commit is a fresh one)
            H.single_prim(ctx, "sphere")
    ctx.clear()                                                    # a graph without objects is refused by the flattener too, and replaces as little
    with pytest.raises(ft.FtError) as e:
        ctx.commit()
    assert e.value.status == -5 and ctx.scene_info() == before
    T.build_lights_scene(ctx, soft=(15,), samples=255)             # and at the limits the same scenes are taken
    T.build_lights_scene(ctx, n_lights=16)
    ctx.clear()
    ctx.set_objects(ctx.group([T.build_tree(ctx, T.right_deep(8, 0, T.x_group))]))
    ctx.commit()
    ctx2 = ft.Context(host_only=True)                              # no commit before the refused one: there is nothing to fall back to
    _refused(lambda: T.build_lights_scene(ctx2, n_lights=17), "16 lights")
    assert _info_or_status(ctx2) == -5
    ctx.close(); ctx2.close()


def test_stack_capacity_is_exactly_255_and_its_rays_cross_what_they_claim():
    ctx = ft.Context(host_only=True)
    ctx.set_option("csg_mesh_capacity", T.STACK_N)
    T.build_stack(ctx)
    assert ctx.scene_info()["csg_capacity"] == 255                 # sphere 2 + square 1 + mesh 251 + circle 1 + empty group 0
    assert ctx.scene_info()["triangles"] == T.STACK_N
    ctx.close()
    o, d = T.stack_rays(STACK_KS)
    assert T.crossings(T.stack_triangles(), o, d).tolist() == list(STACK_KS) + [0, 0, 0, 0]      # in numpy: no tracer involved
    # the oracle agrees, and under exclude it keeps every hit: the ray through everything ends with a list of 255
    counts = stack_reference()["all"][0]
    assert counts[:len(STACK_KS)].tolist() == [k + 4 for k in STACK_KS] and counts[len(STACK_KS) - 1] == 255
    hits = stack_reference()["closest"][0]
    assert hits[:len(STACK_KS)].all() and 0.2 < hits[len(STACK_KS) + 4:].mean() < 1.0


def test_each_light_is_blocked_where_it_should_be_and_the_oracle_agrees():
    """The geometry of the sixteen-light scene by segment-sphere tests in numpy; then the hand-derived colours on the oracle, with
    hard lights and with lights 7, 8 and 15 soft at 255 samples (umbra: 255 of 255 occluded; open: 0)."""
    L, C = T.light_directions(), T.light_colours()
    assert np.allclose(np.linalg.norm(L, axis=1), 1.0)
    for a in range(16):
        for b in range(a):
            assert np.linalg.norm(L[a] - L[b]) > 0.05 and (np.abs(C[a] - C[b]) > 1e-3).all()
    pts = T.light_points()
    blocked = T.blocked_matrix(pts)
    assert np.array_equal(blocked[:16], np.eye(16, dtype=np.int64))                 # P_k: light k alone
    assert blocked[16].sum() == 0 and np.nonzero(blocked[17])[0].tolist() == [3, 12]
    sure = T.blocked_matrix(pts, spread=T.SOFT_SCATTER)                             # whatever direction within the scatter a sample takes
    assert np.array_equal(sure, 2 * blocked - 1)
    want = T.expected_colours(blocked)
    assert len({tuple(np.round(w, 9)) for w in want}) == len(want)
    o, d = T.rays_onto(pts)
    for soft in ((), T.SOFT):
        orc = O.Oracle()
        T.build_lights_scene(orc, soft=soft)
        assert np.array_equal(orc.closest(o, d)[0], np.ones(len(pts), dtype=np.int32))
        assert np.allclose(orc.colour_for_ray(o, d), want, rtol=1e-9, atol=1e-15), soft


def test_deep_reflection_levels_are_alive_on_the_oracle():
    """One light, so the reference's tree of one reflection per light per hit stays a chain.  Level 16 must change pixels against level
    15 (and rays), or the levels above 8 would be dead weight in every comparison below."""
    for fancy in (False, True):
        ref = mirror_reference(fancy)
        assert (ref[16]["frame"] != ref[15]["frame"]).any(axis=2).sum() >= 100
        assert H.pixel_errors(ref[16]["frame"], ref[15]["frame"]).max() > 10 * H.PIXEL_RTOL
        assert (ref[16]["rays"] != ref[15]["rays"]).any(axis=1).sum() >= 200
        counts = [ref[k]["stats"]["rays_traced"] for k in (8, 9, 12, 15, 16)]
        assert counts == sorted(set(counts)), "every further level traces more rays"
        assert not np.isnan(ref[16]["frame"]).any() and not np.isnan(ref[16]["rays"]).any()


# =============================================================================================================================
# GPU half

@gpu
@pytest.mark.parametrize("name", CSG_NAMES)
def test_csg_chain_matches_oracle(hip, name):
    ref = csg_reference(name)
    T.build_csg_case(hip, name)
    H.assert_hits_match(hip.closest(ref["o"], ref["d"]), ref["closest"], rtol=H.TIGHT, what=name)
    assert np.array_equal(hip.blocked(ref["o"], ref["d"], ref["md"]), ref["blocked"]), f"{name}: lightIsBlocked differs"
    got, st = hip.render(_cam(T.CSG_CAMERA), 64, 48, 2, JIT2)
    _frames_match(got, ref["frame"], name)
    assert st["rays_reference_equivalent"] == ref["stats"]["rays_traced"] and st["csg_overflow"] == 0


@gpu
@pytest.mark.parametrize("which", list(ONION))
def test_onion_closed_form_on_the_device(hip, which):
    _check_onion(hip, which)


@gpu
def test_hit_lists_and_marks_of_255(hip):
    """A list of 255 entries (folded over the LDS columns of 8 lanes), a mark of 254 under the circle and one of 255 under the empty
    group; then 256 is refused and the frame of the scene before it comes out bit for bit as it did."""
    ref = stack_reference()
    cam = _cam(STACK_CAMERA, 32 / 24)
    hip.set_option("csg_mesh_capacity", T.STACK_N)
    hip.set_option("csg_auto_grow", 0)                              # an overflow here is a failure, not a reason to grow
    try:
        T.build_stack(hip)
        assert hip.scene_info()["csg_capacity"] == 255
        H.assert_hits_match(hip.closest(ref["o"], ref["d"]), ref["closest"], rtol=H.TIGHT, what="stack")
        assert np.array_equal(hip.blocked(ref["o"], ref["d"], ref["md"]), ref["blocked"])
        got, st = hip.render(cam, 32, 24, 1, ft.jitter_pattern(1))
        _frames_match(got, ref["frame"], "stack")
        assert st["csg_overflow"] == 0 and st["rays_reference_equivalent"] == ref["stats"]["rays_traced"]
        hip.set_option("csg_mesh_capacity", T.STACK_N + 1)
        _refused(lambda: T.build_stack(hip, T.STACK_N + 1), "255 hits")
        assert hip.scene_info()["csg_capacity"] == 255
        again, st2 = hip.render(cam, 32, 24, 1, ft.jitter_pattern(1))
        assert np.array_equal(again, got) and st2["rays_traced"] == st["rays_traced"]
    finally:
        hip.set_option("csg_auto_grow", 1)
        hip.set_option("csg_mesh_capacity", 32)


@gpu
def test_sixteen_lights_closed_form_on_the_device(hip):
    """One byte per light: any swap, shift or carry between the bytes of vis_lo / vis_hi changes a colour, since the lights' colours
    differ pairwise.  Soft: byte 7 is the top of vis_lo, bytes 8 and 15 the ends of vis_hi, each 0xFF in the umbra."""
    pts = T.light_points()
    want = T.expected_colours(T.blocked_matrix(pts))
    o, d = T.rays_onto(pts)
    for soft in ((), T.SOFT):
        T.build_lights_scene(hip, soft=soft)
        got = hip.colour_for_ray(o, d)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-15), (soft, np.abs(got - want).max(axis=1))
    frame, _ = hip.render(_cam(LIGHTS_CAMERA, 48 / 32), 48, 32, 1, ft.jitter_pattern(1), seed=1234)
    for attempt, words in ((lambda: T.build_lights_scene(hip, n_lights=17), ("16 lights",)), (lambda: T.build_lights_scene(hip, soft=(15,), samples=256), ("255 samples",))):
        _refused(attempt, *words)
        again, _ = hip.render(_cam(LIGHTS_CAMERA, 48 / 32), 48, 32, 1, ft.jitter_pattern(1), seed=1234)
        assert np.array_equal(again, frame), "the commit before the refused one is rendered as before"


LIGHTS_CAMERA = ((0.5, 7.0, -3.5), (0.0, 0.0, 0.0), (0, 1, 0), 50.0)
PENUMBRA_SCATTER = 0.25                                           # radians: penumbrae wider than the sphere, where the closed-form scenes have hairlines


@functools.lru_cache(maxsize=None)
def penumbra_reference():
    orc = O.Oracle()
    T.build_lights_scene(orc, soft=T.SOFT, samples=255, scatter=PENUMBRA_SCATTER)
    cam = _cam(LIGHTS_CAMERA, 48 / 32)
    return [orc.render(cam, 48, 32, 2, JIT2, seed=seed) for seed in (1234, 99)]


def test_penumbra_pixels_depend_on_the_stream():
    (a, _), (b, _) = penumbra_reference()
    assert 20 <= (a != b).any(axis=2).sum() <= 48 * 32 // 2, "penumbra pixels, and not everywhere"


@gpu
def test_penumbra_of_255_samples_matches_oracle(hip):
    """Counts between 0 and 255: the frame against the oracle drawing the same streams."""
    T.build_lights_scene(hip, soft=T.SOFT, samples=255, scatter=PENUMBRA_SCATTER)
    for seed, (want, ost) in zip((1234, 99), penumbra_reference()):
        got, st = hip.render(_cam(LIGHTS_CAMERA, 48 / 32), 48, 32, 2, JIT2, seed=seed)
        _frames_match(got, want, f"penumbra, seed {seed}")
        assert st["rays_reference_equivalent"] == pytest.approx(ost["rays_traced"], rel=1e-12)


@gpu
def test_mixed_scene_with_sixteen_lights(hip):
    orc = O.Oracle()
    T.build_mixed_lights(orc)
    cam = ft.make_camera((1.0, 3.0, -7.0), (-0.5, 0.0, 0.0), (0, 1, 0), H.deg(55.0), 64 / 48)
    want, ost = orc.render(cam, 64, 48, 2, JIT2)
    got, st = render_three(hip, T.build_mixed_lights, cam, 64, 48, 2)   # grid, tree and BVH shadows: bitwise the same frame and counts
    _frames_match(got, want, "16 mixed lights")
    assert st["rays_reference_equivalent"] == pytest.approx(ost["rays_traced"], rel=1e-12)
    assert st["rays_shadow"] > 16 * 64 * 48


@gpu
@pytest.mark.parametrize("fancy", [False, True], ids=["mirrors", "fancy"])
def test_max_depth_9_to_16(hip, fancy):
    ref = mirror_reference(fancy)
    T.build_mirror_hall(hip, fancy)
    cam = _cam(T.MIRROR_CAMERA, 48 / 32)
    jit = ft.jitter_pattern(1)
    blocking = {}
    for depth in T.DEPTHS:
        rays = hip.colour_for_ray(ref["o"], ref["d"], max_depth=depth)
        _frames_match(rays[:, None, :], ref[depth]["rays"][:, None, :], f"rays, max_depth {depth}")
        got, st = hip.render(cam, 48, 32, 1, jit, max_depth=depth)
        _frames_match(got, ref[depth]["frame"], f"frame, max_depth {depth}")
        assert st["rays_reference_equivalent"] == ref[depth]["stats"]["rays_traced"], depth
        blocking[depth] = (got, st)
    assert not np.array_equal(blocking[16][0], blocking[15][0])
    # two frames in flight
    with ft.PinnedArray((len(T.DEPTHS), 32, 48, 3)) as pinned:
        pinned[:] = -1.0
        for k, depth in enumerate(T.DEPTHS):
            hip.render_enqueue(cam, 48, 32, 1, jit, max_depth=depth, out=pinned[k])
        hip.wait()
        for k, depth in enumerate(T.DEPTHS):
            assert np.array_equal(pinned[k], blocking[depth][0]), depth
    # every way of cutting the levels: no pixel and no count moves
    keys = ("rays_shadow", "rays_reflect", "rays_traced", "hits_total", "rays_reference_equivalent")
    try:
        for hint, few in ((0, -1), (1, 0), (1, 1000), (1, 10 ** 9)):
            hip.set_option("level_hint", hint)
            hip.set_option("follow_below", few)
            for depth in (9, 16):
                hip.render(cam, 48, 32, 1, jit, max_depth=depth)     # sets the hint under these options
                got, st = hip.render(cam, 48, 32, 1, jit, max_depth=depth)
                assert np.array_equal(got, blocking[depth][0]), (hint, few, depth)
                for key in keys:
                    assert st[key] == blocking[depth][1][key], (hint, few, depth, key)
    finally:
        hip.set_option("level_hint", 1)
        hip.set_option("follow_below", -1)


@gpu
def test_max_depth_17_is_refused_and_leaves_a_queued_frame_intact(hip):
    T.build_mirror_hall(hip, False)
    cam = _cam(T.MIRROR_CAMERA, 48 / 32)
    jit = ft.jitter_pattern(1)
    want, _ = hip.render(cam, 48, 32, 1, jit, max_depth=16)
    o, d = T.mirror_rays(64)
    with ft.PinnedArray((32, 48, 3)) as pinned:
        pinned[:] = -1.0
        hip.render_enqueue(cam, 48, 32, 1, jit, max_depth=16, out=pinned)
        _refused(lambda: hip.render_enqueue(cam, 48, 32, 1, jit, max_depth=17), "16")
        _refused(lambda: hip.render(cam, 48, 32, 1, jit, max_depth=17), "16")
        _refused(lambda: hip.progressive_begin(cam, 48, 32, max_depth=17), "16")
        _refused(lambda: hip.colour_for_ray(o, d, max_depth=17), "16")
        hip.wait()
        assert np.array_equal(pinned, want)
    again, _ = hip.render(cam, 48, 32, 1, jit, max_depth=16)
    assert np.array_equal(again, want)

"""Option "classify_reuse": a classified frame whose slot still holds the classification of the same scene commit, frame size, tiles,
camera, jitter extent and list leaf launches neither k_classify nor k_block_lists, and only the windows of its pixel list that hold
active pixels.  Nothing a caller sees may move with it: every frame here is compared bit for bit, and every ft_stats field but the
times, with the same request rendered by a second context on which the option is 0 for good.

What ran is asserted through Context.classify_reuse(), against the rule the option is defined by, kept here as a model: a context has
four frame slots taken in turn; a slot keeps the key of the last plain classified frame queued into it; a frame reuses exactly when
its slot keeps its own key; commits and the three options that decide a classification drop everything kept."""
import math
from dataclasses import dataclass, replace

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd._capi import LIST_NONE, FtError
from tests import helpers as H
from tests.test_light_space_shadows import bunny_tris

K_SLOTS = 4
W, HH, SPP = 256, 192, 2
JIT = ft.jitter_pattern(SPP)
CAM_A = ft.make_camera((0.0, 0.9, -7.0), (0.6, 0.8, 0.0), (0, 1, 0), H.deg(40.0))     # the two views of
CAM_B = ft.make_camera((0.0, 0.9, -7.0), (-0.9, 0.6, 0.0), (0, 1, 0), H.deg(40.0))    # test_zero_fill_skip_and_classification_ahead_change_no_pixel
CAM_AWAY = ft.make_camera((0.0, 0.9, -7.0), (0.0, 0.9, -20.0), (0, 1, 0), H.deg(40.0))   # the mesh behind the camera: no block is active
CAMS = {"A": CAM_A, "B": CAM_B, "away": CAM_AWAY}
TRIS = np.asarray(bunny_tris(), dtype=np.float64).reshape(-1, 9)


@dataclass(frozen=True)
class Spec:
    """One request.  `classified`: the host classifies it (not a corner-sampled frame, a focus camera or an unbounded scene)."""
    cam: str = "A"
    w: int = W
    h: int = HH
    spp: int = SPP
    scale: float = 1.0            # of the jitter pattern: its extent is max(1, largest |offset| x scale)
    pattern: int = ft.DEFAULT_SEED
    tiles: tuple = None
    rgba8: bool = False
    max_depth: int = ft.MAX_DEPTH
    seed: int = ft.DEFAULT_SEED
    classified: bool = True

    def jitter(self):
        return ft.jitter_pattern(self.spp, seed=self.pattern) * self.scale if self.spp else None

    def extent(self):
        return max(1.0, float(np.abs(self.jitter()).max())) if self.spp else 1.0


A, B = Spec(), Spec(cam="B")


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


def bunny_ops(shift=(0.0, 0.0, 0.0)):
    return [("scale", (8.0, 8.0, 8.0)), ("rotate", (0, 1, 0), math.pi), ("translate", shift)]   # scenes/bunny.scene, then the shift


def lower_bunny(ctx):
    """scenes/bunny.scene through the builder, so that the mesh and its transform can be edited.  Returns (mesh node, transform node)."""
    ctx.clear()
    mesh = ctx.bsp_mesh(0, TRIS)
    xf = ctx.transform(bunny_ops(), mesh)
    ctx.set_objects(ctx.group([ctx.material(xf, colour=(0.8, 0.7, 0.6))]))
    ctx.add_directional((-3, -2, 3), (1, 1, 1))
    ctx.commit()
    return mesh, xf


def lower_csg(ctx):
    """Small and bounded, under CSG and reflective: a frame of it is classified, carries no lists, and follows max_depth."""
    ctx.clear()
    shell = ctx.subtract(ctx.primitive(ft.CUBE), ctx.scale((0.65, 0.65, 0.65), ctx.primitive(ft.SPHERE)))
    items = [ctx.material(ctx.translate((0.6, 0.8, 0.0), shell), colour=(1, 0.2, 0.1), reflectance=0.4, shineyness=10),
             ctx.material(ctx.translate((-0.8, 0.8, 0.6), ctx.primitive(ft.SPHERE)), colour=(0.1, 0.4, 1), reflectance=0.4, shineyness=10)]
    ctx.set_objects(ctx.group(items))
    ctx.add_positional((0, 3, -6), (1, 0.01, 0.02), (1, 1, 1))
    ctx.commit()


def lower_inside(ctx):
    """The camera inside a hollow sphere: every block is active."""
    ctx.clear()
    shell = ctx.subtract(ctx.scale((11, 11, 11), ctx.primitive(ft.SPHERE)), ctx.scale((10, 10, 10), ctx.primitive(ft.SPHERE)))
    ctx.set_objects(ctx.group([ctx.material(shell, colour=(0.4, 0.4, 0.4)), ctx.material(ctx.translate((0.6, 0.8, 0), ctx.primitive(ft.CUBE)), colour=(1, 0, 0))]))
    ctx.add_positional((0, 0, -8), (1, 0.01, 0.02), (1, 1, 1))
    ctx.commit()


def lower_ground(ctx):
    ctx.clear()
    ctx.set_objects(ctx.group([ctx.primitive(ft.PLANE), ctx.translate((0.6, 0.8, 0), ctx.primitive(ft.SPHERE))]))
    ctx.add_directional((0, -1, 0.5), (1, 1, 1))
    ctx.commit()


class Rig:
    """The context under test, its twin with "classify_reuse" = 0, and the model of what the slots keep."""

    def __init__(self):
        self.ctx, self.ref = ft.Context(0), ft.Context(0)
        self.ref.set_option("classify_reuse", 0)
        for c in (self.ctx, self.ref):
            c.set_option("level_hint", 0)        # n_launches then does not depend on which frames of a signature came before
        self.kept, self.turn, self.serial = [None] * K_SLOTS, 0, 0
        self.opts = {"classify_pixels": 1, "primary_block_lists": 1, "classify_reuse": 1}
        self.refs = {}

    def close(self):
        self.ctx.close()
        self.ref.close()

    def both(self, fn):
        """A commit (or any edit that ends in one) on both contexts: everything kept is dropped, references start over."""
        out = fn(self.ctx)
        fn(self.ref)
        self.serial += 1
        self.kept = [None] * K_SLOTS
        return out

    def option(self, key, value):
        self.ctx.set_option(key, value)
        if key != "classify_reuse":
            self.ref.set_option(key, value)
        self.opts[key] = value
        self.kept = [None] * K_SLOTS

    def key(self, s):
        if not (s.classified and s.spp and self.opts["classify_pixels"]):
            return None
        return (self.serial, s.cam, s.w, s.h, s.tiles, s.extent(), bool(self.opts["primary_block_lists"]))

    def slot(self, key):
        """The model: the frame takes the next slot; returns whether it finds its own key there."""
        hit = key is not None and self.kept[self.turn] == key and bool(self.opts["classify_reuse"])
        if not hit:
            self.kept[self.turn] = key
        self.turn = (self.turn + 1) % K_SLOTS
        return hit

    @staticmethod
    def render(ctx, s):
        fn = ctx.render_rgba8 if s.rgba8 else ctx.render
        return fn(CAMS[s.cam], s.w, s.h, s.spp, s.jitter(), max_depth=s.max_depth, seed=s.seed, tiles=list(s.tiles) if s.tiles else None)

    def reference(self, s):
        at = (self.serial, tuple(sorted((k, v) for k, v in self.opts.items() if k != "classify_reuse")), s)
        if at not in self.refs:
            img, st = self.render(self.ref, s)
            self.refs[at] = (img, counters(st))
        return self.refs[at]

    @staticmethod
    def region(s, img):
        return img if not s.tiles else np.concatenate([img[y0:y0 + h, x0:x0 + w].reshape(-1, img.shape[-1]) for x0, y0, w, h in s.tiles])

    def expect(self, s, before):
        """The counts since `before` against the model, for the frame of `s` just queued.  Returns whether it reused."""
        hit = self.slot(self.key(s))
        now = self.ctx.classify_reuse()
        assert now["reused"] - before["reused"] == int(hit), (s, hit)
        assert now["classified"] - before["classified"] == int(self.key(s) is not None and not hit), (s, hit)
        return hit

    def frame(self, s):
        """A blocking frame of `s`: equal to the reference, every counter too, and reused exactly when the model says so."""
        want, want_st = self.reference(s)
        before = self.ctx.classify_reuse()
        img, st = self.render(self.ctx, s)
        hit = self.expect(s, before)
        assert np.array_equal(self.region(s, img), self.region(s, want)), (s, hit)
        assert counters(st) == want_st, (s, hit)
        return hit

    def frames(self, specs):
        return sum(self.frame(s) for s in specs)

    def queued(self, specs):
        """The same frames queued, each copied out behind its last kernel; the last one's statistics are compared."""
        n_hits = 0
        shape = lambda s: (s.h, s.w, 4 if s.rgba8 else 3)
        outs = [ft.PinnedArray(shape(s), dtype=np.uint8 if s.rgba8 else np.float64) for s in specs]
        try:
            for s, out in zip(specs, outs):
                out.array[:] = 0
                before = self.ctx.classify_reuse()
                self.ctx.render_enqueue(CAMS[s.cam], s.w, s.h, s.spp, s.jitter(), max_depth=s.max_depth, seed=s.seed, tiles=list(s.tiles) if s.tiles else None,
                                        rgba8=s.rgba8, out=out.array)
                n_hits += self.expect(s, before)
            st = self.ctx.wait()
            for s, out in zip(specs, outs):
                assert np.array_equal(self.region(s, out.array), self.region(s, self.reference(s)[0])), s
            assert counters(st) == self.reference(specs[-1])[1]
        finally:
            for out in outs:
                out.close()
        return n_hits


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


# ------------------------------------------------------------------------------------------------------------------------ 1, 2, 4
@pytest.mark.gpu
def test_held_view_queued_then_blocking(rig):
    rig.both(lower_bunny)
    n = 2 * K_SLOTS + 1
    assert rig.queued([A] * n) == n - K_SLOTS            # the first kSlots frames after a commit classify, every later one reuses
    assert rig.frames([A] * n) == n
    img = rig.reference(A)[0]
    seen = np.abs(img).sum(axis=-1) > 0
    assert seen.any() and (~seen).mean() > 0.5                 # sparse: a stale map would show


@pytest.mark.gpu
def test_new_pattern_and_seed_every_frame_reuse(rig):
    rig.both(lower_bunny)
    specs = [replace(A, pattern=100 + k, seed=7 + k) for k in range(2 * K_SLOTS + 1)]
    assert len({s.jitter().tobytes() for s in specs}) == len(specs) and {s.extent() for s in specs} == {1.0}
    assert rig.frames(specs) == len(specs) - K_SLOTS
    assert rig.queued(specs) == len(specs)
    refs = [rig.reference(s)[0] for s in specs]
    assert not np.array_equal(refs[0], refs[1])               # each frame has a reference of its own


@pytest.mark.gpu
def test_lists_after_a_warm_frame_are_the_cold_frames(rig):
    rig.both(lower_bunny)
    rig.render(rig.ref, A)
    want = rig.ref.block_lists()
    assert rig.frames([A] * (K_SLOTS + 1)) == 1
    got = rig.ctx.block_lists()
    assert want["leaf"] >= 0 and len(want["heads"]) > 0 and want["entries"].size > 0
    assert got["leaf"] == want["leaf"] and got["capacity"] == want["capacity"]
    for k in ("pos_block", "plane"):
        assert np.array_equal(got[k], want[k]), k
    # where a block's entries lie in the pool is decided by the order its wave reached the cursor in: the lists are compared block by block
    assert np.array_equal(got["heads"] == LIST_NONE, want["heads"] == LIST_NONE) and (want["heads"] != LIST_NONE).any()
    assert got["entries"].size == want["entries"].size
    for pos, (g, w) in enumerate(zip(got["heads"], want["heads"])):
        if w != LIST_NONE:
            assert (g & 127) == (w & 127) and np.array_equal(got["entries"][g >> 7:(g >> 7) + (g & 127)], want["entries"][w >> 7:(w >> 7) + (w & 127)]), pos
    # kSlots warm frames later the same slot is the last one queued again: its buffers are, word for word, as they were
    assert rig.frames([A] * K_SLOTS) == K_SLOTS
    again = rig.ctx.block_lists()
    for k in ("heads", "pos_block", "entries"):
        assert np.array_equal(again[k], got[k]), k


# ------------------------------------------------------------------------------------------------------------------------------ 3
def around(rig, other, n=K_SLOTS + 1, rounds=2):
    """A x n, then `other` (a Spec, or a callable that does something else), again, and A to the end: whatever `other` is, it lands
    in a slot that keeps A's key, and the A frames behind it find three slots that still do."""
    hits = 0
    for _ in range(rounds):
        hits += rig.frames([A] * n)
        hits += rig.frame(other) if isinstance(other, Spec) else (other() or 0)
    return hits + rig.frames([A] * n)


FRAME_CASES = {
    "camera": (B, False),
    "tiles": (replace(A, tiles=((0, 0, 128, 192),)), False),
    "two tiles": (replace(A, tiles=((0, 0, 128, 192), (128, 64, 64, 64))), False),
    "resolution": (replace(A, w=128, h=96), False),
    "extent": (replace(A, scale=1.5 / float(np.abs(JIT).max())), False),
    "rgba8": (replace(A, rgba8=True), True),                  # another format reads the same classification, and fills its own buffer's zeros
    "corner": (replace(A, spp=0, classified=False), False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(FRAME_CASES))
def test_a_frame_of_another_kind_in_between(rig, what):
    other, same_key = FRAME_CASES[what]
    rig.both(lower_bunny)
    assert (rig.key(other) == rig.key(A)) == same_key
    if what == "extent":
        assert abs(other.extent() - 1.5) < 1e-12
    hits = around(rig, other)
    assert hits > K_SLOTS                                      # the case does not pass on cold frames alone
    # the other kind twice in a row in one slot's turn and A's after it, queued
    rig.queued([A, other, other, A, A, A, A, other, A, A, A])


@pytest.mark.gpu
def test_max_depth_changes_the_pixels_not_the_classification(rig):
    rig.both(lower_csg)
    shallow = replace(A, max_depth=0)
    assert rig.key(shallow) == rig.key(A)
    hits = around(rig, shallow)
    assert hits == 3 * (K_SLOTS + 1) + 2 - K_SLOTS             # only the first kSlots frames classify
    assert not np.array_equal(rig.reference(A)[0], rig.reference(shallow)[0])
    assert rig.reference(A)[1]["rays_reflect"] > 0 and rig.reference(shallow)[1]["rays_reflect"] == 0
    assert rig.ctx.block_lists()["leaf"] == -1                 # classified without lists


@pytest.mark.gpu
def test_commits_of_every_kind_start_over(rig):
    mesh, xf = rig.both(lower_bunny)
    n = K_SLOTS + 2
    assert rig.frames([A] * n) == 2
    # another scene under the same camera, and back
    rig.both(lower_csg)
    assert rig.frames([A] * n) == 2
    mesh, xf = rig.both(lower_bunny)
    assert rig.frames([A] * n) == 2
    still = rig.reference(A)[0]
    # the mesh moved by several blocks (an 8x8 block is about 0.22 world units wide at the mesh)
    def moved(ctx):
        ctx.set_transform(xf, bunny_ops((1.2, 0.3, 0.0)))
        ctx.commit_moved()
    rig.both(moved)
    assert rig.frames([A] * n) == 2
    assert (np.abs(rig.reference(A)[0] - still).sum(axis=-1) > 0).sum() > 64 * 8
    # ... and its vertices, in model space (x 8 in the world), the other way
    was = rig.reference(A)[0]
    def deformed(ctx):
        ctx.set_mesh_triangles(mesh, TRIS + np.tile([0.3, 0.0, 0.0], 3))
        ctx.commit_deformed()
    rig.both(deformed)
    assert rig.frames([A] * n) == 2
    assert (np.abs(rig.reference(A)[0] - was).sum(axis=-1) > 0).sum() > 64 * 8
    assert rig.queued([A] * n) == n


@pytest.mark.gpu
def test_the_options_that_decide_a_classification(rig):
    n = K_SLOTS + 2
    try:
        rig.both(lower_bunny)
        rig.option("classify_pixels", 0)
        assert rig.frames([A] * n) == 0
        rig.option("classify_pixels", 1)
        assert rig.frames([A] * n) == 2
        for lists in (0, 1, 0):
            rig.option("primary_block_lists", lists)
            assert rig.frames([A] * n) == 2
            assert (rig.ctx.block_lists()["leaf"] >= 0) == bool(lists)
        rig.option("primary_block_lists", 1)
        rig.option("classify_reuse", 0)
        assert rig.frames([A] * n) == 0
        rig.option("classify_reuse", 1)
        assert rig.frames([A] * n) == 2
        rig.option("classify_reuse", 0)                        # set under queued frames that reuse
        rig.option("classify_reuse", 1)
        assert rig.queued([A] * n) == 2
    finally:
        for k in ("classify_pixels", "primary_block_lists", "classify_reuse"):
            rig.option(k, 1)


@pytest.mark.gpu
def test_other_calls_in_between(rig):
    rig.both(lower_bunny)
    o, d = H.random_rays(64, 3, toward=(0.6, 0.8, 0.0))

    def queries():
        rig.ctx.closest(o, d)
        rig.ctx.blocked(o, d, np.full(64, 50.0))

    def accumulation(tolerance):
        def run():
            rig.ctx.progressive_begin(CAM_A, W, HH, tolerance=tolerance, min_samples=2)
            for k in range(3):
                rig.ctx.progressive_pass(SPP, ft.jitter_pattern(SPP, seed=11 + k), seed=k)
                rig.slot(None)                                 # a pass takes a slot and keeps nothing in it
            rig.ctx.progressive_end()
        return run

    def surfaces():
        rig.ctx.render_aov(CAM_A, W, HH, SPP, JIT, channels=["leaf"])      # its own buffers: no slot

    full = 3 * (K_SLOTS + 1) - K_SLOTS
    assert around(rig, queries) == full
    rig.both(lower_bunny)
    assert around(rig, surfaces) == full
    rig.both(lower_bunny)
    assert around(rig, accumulation(0.0)) == full - 2 * 3      # each round's three passes cost three of the slots their A frames
    rig.both(lower_bunny)
    assert around(rig, accumulation(0.05)) == full - 2 * 3     # adaptive passes classify into the slots' buffers themselves


# ------------------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.gpu
def test_warm_frames_launch_only_the_windows_that_hold_work(rig):
    chunk = 3072                                               # classified windows are cut from 5 x this: 7680 pixels at 2 spp, evened to 7040
    per = 7040
    try:
        for c in (rig.ctx, rig.ref):
            c.set_option("chunk_samples", chunk)
        cold_windows = -(-W * HH // per)
        assert cold_windows >= 6
        for lower, s, check in ((lower_bunny, A, "sparse"), (lower_inside, A, "full"), (lower_bunny, replace(A, cam="away"), "empty")):
            rig.both(lower)
            want, st = rig.reference(s)
            assert st["n_chunks"] == cold_windows
            n_active = W * HH - st["rays_primary_culled"] // SPP
            holding = max(1, -(-n_active // per))              # (a frame without an active pixel still launches one window: the zero fill and the report)
            if check == "sparse":
                assert n_active % 64 == 0 and 0 < n_active and holding <= 3
            elif check == "full":
                assert n_active == W * HH and holding == cold_windows
            else:
                assert n_active == 0 and not want.any() and st["rays_traced"] == 0
            before = rig.ctx.classify_reuse()
            assert rig.frames([s] * (K_SLOTS + 3)) == 3        # n_chunks and n_launches are compared with the reference's in there
            assert rig.queued([s] * 3) == 3
            now = rig.ctx.classify_reuse()
            assert now["windows_skipped"] - before["windows_skipped"] == 6 * (cold_windows - holding), check
            assert now["windows_launched"] - before["windows_launched"] == K_SLOTS * cold_windows + 6 * holding, check
    finally:
        for c in (rig.ctx, rig.ref):
            c.set_option("chunk_samples", 16 << 20)


# ------------------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.gpu
def test_frames_the_host_does_not_classify_never_reuse(rig):
    rig.both(lower_ground)
    unbounded = replace(A, classified=False)
    before = rig.ctx.classify_reuse()
    assert rig.frames([unbounded] * (2 * K_SLOTS + 1)) == 0
    rig.both(lower_bunny)
    focus = ft.make_camera((0.0, 0.9, -7.0), (0.6, 0.8, 0.0), (0, 1, 0), H.deg(40.0))
    focus.has_focus, focus.focal_length, focus.aperture_angular_size = 1, 7.0, H.deg(0.5)
    CAMS["focus"] = focus
    assert rig.frames([replace(A, cam="focus", classified=False)] * (2 * K_SLOTS + 1)) == 0
    now = rig.ctx.classify_reuse()
    assert now["reused"] == before["reused"] and now["classified"] == before["classified"]


# ------------------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.gpu
def test_two_devices_keep_their_own_records(rig):
    rig.both(lower_bunny)
    want, want_st = rig.reference(A)
    two = ft.Context(device=[0, 0])
    try:
        two.set_option("level_hint", 0)
        lower_bunny(two)
        assert two.classify_reuse() == dict(classified=0, reused=0, windows_launched=0, windows_skipped=0)
        n = 2 * K_SLOTS + 1
        for k in range(n):
            img, st = two.render(CAM_A, W, HH, SPP, JIT)
            assert np.array_equal(img, want), k
            got = two.classify_reuse()                         # each device takes its 12 bands of every frame into its own slots
            assert (got["classified"], got["reused"]) == (2 * min(k + 1, K_SLOTS), 2 * max(0, k + 1 - K_SLOTS)), k
        for k in ("rays_primary", "rays_primary_culled", "hits_primary", "rays_shadow", "rays_traced"):
            assert st[k] == want_st[k], k
    finally:
        two.close()


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_the_option_is_a_flag_on_a_host_only_context():
    ctx = ft.Context(host_only=True)
    try:
        for v in (0, 1, 7, -3, 1 << 40):
            ctx.set_option("classify_reuse", v)
    finally:
        ctx.close()


def test_the_counts_need_a_device():
    ctx = ft.Context(host_only=True)
    try:
        with pytest.raises(FtError) as e:
            ctx.classify_reuse()
        assert e.value.status == -2
        with pytest.raises(FtError) as other:                   # as the other device queries
            ctx.block_lists()
        assert other.value.status == e.value.status
    finally:
        ctx.close()

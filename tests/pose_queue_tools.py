"""Queued pose and light commits (ft_scene_commit_moved_enqueue / ft_scene_commit_lights_enqueue): the sequences of
tests/test_pose_queue.py over the scenes of tests/move_tools.py and tests/shadow_tools.py, and the oracle's view of each.

A sequence is a list of steps {"pose": ..., "lights": ...}: the transform lists of every moving node (move_tools' pose) and, for the
lights sequences, every light of the scene (light_tools' form).  All of them can be QUEUED whatever "light_space_shadows" says: the mesh
leaves only slide, no directional light turns."""
import functools

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import light_tools as L
from . import move_tools as MV
from . import shadow_tools as S
from . import walk_tools as W
from . import test_temporal_motion as M

STEPS = 12                      # more than the pose sets a device may hold (9): sets are reused while frames are in flight
FRAME_SLOTS = 4                 # ft_context::kSlots: a device's frames in flight
MIN_CHANGED = 20
SLIDES, LIGHTS, HAND = "multi-leaf", "multi-leaf lights", MV.HAND
SEQUENCES = (SLIDES, HAND, LIGHTS)


def scene_of(seq):
    return HAND if seq == HAND else "multi-leaf"


def _slid(k):
    """multi-leaf with both moving casters slid by a step-dependent fraction of their radius: -0.30 .. 0.36 in steps of 0.06."""
    case = S.CASES["multi-leaf"]
    pose = MV.base_pose(case)
    f = -0.36 + 0.06 * k
    for part in MV.MOVERS["multi-leaf"]:
        _, r = MV.centre_of(case, part)
        pose[part] = pose[part] + [("translate", (f * r, 0.0, -0.6 * f * r))]
    return pose


def _lit(k):
    """multi-leaf's lights at step k: the point light along a line, one directional light's colour (its direction stays), the soft light's
    scatter and colour (its direction stays too)."""
    base = L.initial(S.CASES["multi-leaf"])
    out = list(base)
    first_dir = True
    for i, l in enumerate(base):
        if l[0] == "point":
            out[i] = ("point", tuple(float(x) for x in np.asarray(l[1]) + k * np.array([0.3, 0.1, -0.2])), l[2], l[3])
        elif l[0] == "soft":
            out[i] = ("soft", l[1], l[2], l[3] * (1.0 + 0.1 * k), tuple(float(x) for x in np.asarray(l[4]) * (1.0 - 0.03 * k)))
        elif first_dir:
            out[i] = ("dir", l[1], (1.0 - 0.04 * k, 1.0, 0.6 + 0.03 * k))
            first_dir = False
    return out


def _hand(k):
    """The hand scene of test_temporal_motion.py at call k with its mesh sliding only: the sphere slides, the cube turns and stretches, the
    CSG operand moves - primitives, whose turns touch no light-space pair."""
    pose = M._pose(float(k))
    still = M._pose(0.0)["mesh"]
    pose["mesh"] = still[:2] + [("translate", (-4.9 + 0.05 * k, 3.2, 0.5))]
    return pose


@functools.lru_cache(maxsize=None)
def sequence(seq):
    """Step 0 (the committed scene) and STEPS steps."""
    if seq == SLIDES:
        return [dict(pose=_slid(k) if k else MV.base_pose(S.CASES["multi-leaf"]), lights=None) for k in range(STEPS + 1)]
    if seq == LIGHTS:
        return [dict(pose=_slid(k) if k else MV.base_pose(S.CASES["multi-leaf"]), lights=_lit(k)) for k in range(STEPS + 1)]
    return [dict(pose=_hand(k), lights=None) for k in range(STEPS + 1)]


def build(b, seq, step):
    """The scene of a sequence at `step`, built from scratch and committed; returns the handles."""
    name = scene_of(seq)
    if name == HAND:
        return M._build(b, step["pose"])
    return MV.build(b, S.CASES[name], step["pose"], lights=step["lights"])


def set_step(ctx, hd, step):
    """The setters of a step, the lights first - each followed by its queued commit (a pending light setter sends the moved call to the
    full commit, a pending transform makes the lights call refuse)."""
    if step["lights"] is not None:
        L.set_lights(ctx, step["lights"])
        ctx.commit_lights_enqueue()
    MV.move(ctx, hd, step["pose"], commit=False)
    ctx.commit_moved_enqueue()


def frame_args(seq, spp):
    """(camera, res_h, res_v, spp, jitter) and the tiles of a sequence's frames."""
    if scene_of(seq) == HAND:
        return (M._camera(), M.W, M.Hh, spp, S.jitter(spp)), None
    view = S.view_of(S.CASES["multi-leaf"])
    return (W.camera(view), view.w, view.h, spp, S.jitter(spp)), view.tiles


@functools.lru_cache(maxsize=None)
def oracle_frames(seq, lights_only=False):
    """The oracle's 1-sample frame of every step; lights_only: with the objects left at step 0's pose."""
    steps = sequence(seq)
    args, tiles = frame_args(seq, 1)
    out = []
    for step in steps:
        orc = O.Oracle()
        build(orc, seq, dict(pose=steps[0]["pose"] if lights_only else step["pose"], lights=step["lights"]))
        frame, _ = orc.render(*args, tiles=tiles)
        orc.close()
        out.append(frame)
    return out


def changed(a, b):
    """Pixels in which two frames differ."""
    return int((np.any(a != b, axis=2) & ~(np.isnan(a).all(axis=2) & np.isnan(b).all(axis=2))).sum())


def pending_at_last_call(frames_queued_before):
    """Frames the host still has pending when the commit of the last step returns, from the frame driver's rule alone: a frame is retired
    by ft_render_wait, by a blocking call, or by the enqueue that takes its slot again - so with one frame queued per step and nothing
    else, every frame queued so far is pending until the FRAME_SLOTS slots are full, and FRAME_SLOTS of them from then on.  A queued commit
    retires none."""
    return min(frames_queued_before, FRAME_SLOTS)

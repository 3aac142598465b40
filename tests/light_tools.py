"""Moving lights (ft_scene_commit_lights) on the shadow cases of tests/shadow_tools.py: the light sequences, scenes whose lights differ
from the case's while receiver and view stay the case's own, the oracle's view of every step, and the checks of what a call leaves in
device memory.

A step is a list of lights in the form shadow_tools.Case.lights has them, with a colour appended: ("dir", v, colour), ("point", p,
falloff, colour), ("soft", v, samples, scatter, colour).  Step 0 is the case as shadow_tools.build commits it."""
import functools
import math

import numpy as np

import functracer_amd as ft
from oracle import ft_oracle_py as O

from . import shadow_tools as S
from . import walk_tools as W
from .test_light_space_grid import check_grid, grid_of
from .test_light_space_shadows import NONE, check_tree, light_space, pair_root

NAMES = ("blob(8)", "blob(65)-xf", "blob(65)-mirror", "concentric", "flat-in-plane", "two_clusters", "identical", "chain(256)", "multi-leaf")
# The tilts in degrees, small and moderate: 2 and 15 unless the case's eye, which looks at a narrow shadow, loses it at that angle
# (test_every_step_casts_shadows_and_changes_the_frame_on_the_oracle states the condition; the counts are in DESIGN.md 17)
TILTS = {"blob(8)": (1.0, 2.0), "blob(65)-mirror": (2.0, 10.0), "concentric": (2.0, 3.0)}
AXIS = (0.0, -1.0, 0.0)
WHITE, TINT = (1.0, 1.0, 1.0), (0.8, 0.9, 1.0)
POINT_COLOUR, POINT_FALLOFF, SOFT_COLOUR = (0.5, 0.5, 1.0), (1.0, 0.0, 0.02), (0.6, 0.6, 0.6)   # shadow_tools.build's
MAX_CELL, ENTRIES_PER_TRI = 256, 16


def tilt(v, angle):
    """v turned by `angle` about an axis perpendicular to it (the cross product with the axis v is least aligned with)."""
    v = np.asarray(v, dtype=np.float64)
    d = v / np.linalg.norm(v)
    k = np.cross(d, np.eye(3)[int(np.argmin(np.abs(d)))])
    k /= np.linalg.norm(k)
    w = np.cross(k, d)                                             # k, d, w orthonormal: turning d about k moves it towards w
    return tuple(float(x) for x in np.linalg.norm(v) * (math.cos(angle) * d + math.sin(angle) * w))


def initial(case):
    """Step 0: the case's lights with the colours shadow_tools.build gives them."""
    out = []
    for l in case.lights:
        if l[0] == "dir":
            out.append(("dir", tuple(float(x) for x in l[1]), WHITE))
        elif l[0] == "point":
            out.append(("point", tuple(float(x) for x in l[1]), POINT_FALLOFF, POINT_COLOUR))
        else:
            out.append(("soft", tuple(float(x) for x in l[1]), l[2], l[3], SOFT_COLOUR))
    return out


@functools.lru_cache(maxsize=None)
def sequence(name):
    """[(what, lights)] of a case, step 0 first.  `a` and `b`: its two directional lights.  The second one carries a tint from step 1 on, so
    that exchanging the directions changes the frame."""
    case = S.CASES[name]
    base = initial(case)
    ia, ib = [k for k, l in enumerate(base) if l[0] == "dir"]
    a, b = base[ia][1], base[ib][1]
    SMALL, MODERATE = (math.radians(x) for x in TILTS.get(name, (2.0, 15.0)))

    def with_dirs(va, vb, lights=None):
        out = list(lights if lights is not None else base)
        out[ia] = ("dir", tuple(va), WHITE)
        out[ib] = ("dir", tuple(vb), TINT)
        return out

    # from here on one light changes at a time: the one that casts less shadow in view, so that the other's shadow stays
    counts = S.shadow_counts(name)
    keep_a = counts[ia][0] >= counts[ib][0]

    def one(v):
        return with_dirs(a, v) if keep_a else with_dirs(v, b)

    other = b if keep_a else a
    steps = [("original", base),
             ("exchanged", with_dirs(b, a)),
             ("tilted a little", with_dirs(tilt(a, SMALL), tilt(b, SMALL))),
             ("tilted further", with_dirs(tilt(a, MODERATE), tilt(b, MODERATE))),
             ("an axis", one(AXIS if tuple(other) != AXIS else (0.0, 0.0, 1.0))),
             ("the diagonal", one(S.DIAGONAL)),
             ("hair", one(S.HAIR)),
             ("zero", one((0.0, 0.0, 0.0))),
             ("usable again", one(tilt(other, MODERATE)))]
    if name == "multi-leaf":
        moved = list(base)
        moved[1] = ("point", (1.0, 5.0, -1.0), (1.0, 0.05, 0.01), (0.9, 0.4, 0.4))
        steps.append(("the point light moved", with_dirs(tilt(a, SMALL), tilt(b, SMALL), moved)))
        moved = list(moved)
        moved[0] = ("soft", (0.2, -2.0, 0.6), base[0][2], 0.09, (0.3, 0.7, 0.5))
        steps.append(("the soft light turned", with_dirs(tilt(a, SMALL), tilt(b, SMALL), moved)))
    steps.append(("original again", base))
    return steps


def add_lights(b, lights):
    for l in lights:
        if l[0] == "dir":
            b.add_directional(l[1], l[2])
        elif l[0] == "point":
            b.add_positional(l[1], l[2], l[3])
        else:
            b.add_soft_directional(l[1], l[2], l[3], l[4])


def build(b, case, lights):
    """shadow_tools.build with other lights: the casters, the receiver and (view_of) the eye stay those of the case's own lights."""
    recv_ops, _ = S.geometry(case)
    b.clear()
    items, node = [], None
    for mesh, ops, kind in case.parts:
        if kind != "same":
            node = b.bsp_mesh(0, S.mesh_tris(mesh).reshape(-1, 9))
        item = b.material(b.transform(list(ops), node) if ops else node, colour=S.MESH_COLOUR)
        items.append(b.ignore_light(item) if kind == "unlit" else item)
    items.append(b.material(b.transform(recv_ops, b.primitive(ft.SQUARE)), colour=S.RECEIVER_COLOUR))
    b.set_objects(b.group(items))
    add_lights(b, lights)
    b.commit()


def set_lights(ctx, lights):
    """The setters for every light of a step (index = position)."""
    for k, l in enumerate(lights):
        if l[0] == "dir":
            ctx.set_directional(k, l[1], l[2])
        elif l[0] == "point":
            ctx.set_positional(k, l[1], l[2], l[3])
        else:
            ctx.set_soft_directional(k, l[1], l[3], l[4])


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}


# ---------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def oracle_steps(name):
    """Per step: (receiver pixels in view that some directional light of the step leaves in shadow, the oracle's 1-sample frame)."""
    case = S.CASES[name]
    view = S.view_of(case)
    out = []
    for what, lights in sequence(name):
        orc = O.Oracle()
        build(orc, case, lights)
        o, d, _, _ = W.pixel_rays(view)
        hit, _, p, n, col = orc.closest(o + S.SLIGHT_OFFSET * d, d)
        hit = hit.astype(bool)
        receiver = hit & (np.abs(col - np.array(S.RECEIVER_COLOUR)).max(axis=1) < 1e-9)
        origin = p + S.SLIGHT_OFFSET * n
        dark = np.zeros(len(hit), dtype=bool)
        for l in lights:
            v = np.asarray(l[1], dtype=np.float64)
            if l[0] != "dir" or not np.linalg.norm(v) > 0.0:
                continue
            dark[receiver] |= orc.blocked(origin[receiver], np.broadcast_to(-v, origin[receiver].shape).copy(), np.full(int(receiver.sum()), 1e300)).astype(bool)
        frame, _ = orc.render(W.camera(view), view.w, view.h, 1, S.jitter(1), tiles=view.tiles)
        orc.close()
        out.append((int(dark.sum()), frame))
    return out


# ---------------------------------------------------------------------------------------------------------------- what a call leaves in HBM
def _entry_boxes(cells):
    """[(box[5] float32, multiplicity)] per distinct triangle record of a grid, from check_grid's cells."""
    seen = {}
    for entries in cells.values():
        here = {}
        for b, t in entries:
            here[t.tobytes()] = (b, here.get(t.tobytes(), (b, 0))[1] + 1)
        for k, v in here.items():
            seen.setdefault(k, v)
    return list(seen.values())


def attempt_rule(boxes, n):
    """build_grid's choice of (s, n_u, n_v) for n triangles with these entry boxes, or None: its own arithmetic, floats as float32."""
    B = np.array([b for b, _ in boxes], dtype=np.float32)
    mult = np.array([m for _, m in boxes], dtype=np.int64)
    Ru = float(np.abs(B[:, 0:2]).max())
    Rv = float(np.abs(B[:, 2:4]).max())
    side = 2.0 * max(Ru, Rv)
    if not side > 0.0:
        return None
    h = max(math.sqrt(4.0 * Ru * Rv / n), side / 1024.0)
    s = np.float32(1.0 / h)
    for _ in range(8):
        if not s > 0:
            return None
        nu = int(min(1024.0, max(1.0, math.ceil(2.0 * Ru * float(s)))))
        nv = int(min(1024.0, max(1.0, math.ceil(2.0 * Rv * float(s)))))
        entries = 0
        for b, m in zip(B, mult):
            entries += int(m) * (S._cell(b[1], s, nu) - S._cell(b[0], s, nu) + 1) * (S._cell(b[3], s, nv) - S._cell(b[2], s, nv) + 1)
        if nu * nv <= 2 * n and entries <= ENTRIES_PER_TRI * n:
            return (float(s), nu, nv) if nu * nv >= 2 else None
        s = np.float32(s * np.float32(0.75))
    return None


def check_structures(ctx, case, lights, grids=True):
    """Every pair of the context as ft_debug_light_space reads it back: the tree holds every triangle of its mesh in boxes that hold it;
    a grid lists every triangle in every cell its box overlaps, is the one build_grid's attempt rule picks for its entry boxes, and
    orders equal w_max by list index; a light without a usable direction has neither.  Returns {(part, light): (n_u, n_v)}."""
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    kinds = {}
    for part, (mesh, ops, kind) in enumerate(case.parts):
        base = int(leaf_pairs[part])
        tris = S.mesh_tris(mesh)
        n = len(tris)
        if n < 8 or kind == "unlit":
            assert base == 0xFFFFFFFF
            continue
        order = {np.concatenate([t[0], t[1] - t[0], t[2] - t[0]]).tobytes(): k for k, t in reversed(list(enumerate(tris.reshape(-1, 3, 3))))}
        for l, light in enumerate(lights):
            rec = pairs[base + l]
            what = f"{case.name} part {part} light {l} {light[1]}"
            if light[0] != "dir" or not np.linalg.norm(light[1]) > 0.0:
                assert pair_root(rec) == NONE and grid_of(rec)[2] == 0, what
                continue
            assert pair_root(rec) >= 0, what
            frame = np.array([rec[0:3], rec[3:6], rec[6:9]])
            assert np.allclose(frame @ frame.T, np.eye(3), atol=1e-14), what
            assert check_tree(rec, nodes, ls_tris) == n, what
            _, s, nu, nv = grid_of(rec)
            kinds[(part, l)] = (nu, nv)
            if nu == 0:
                continue
            assert grids, what
            cells = check_grid(rec, nodes, ls_tris, n)
            assert attempt_rule(_entry_boxes(cells), n) == (s, nu, nv), what
            for key, entries in cells.items():                      # equal w_max: ascending list index
                for (b0, t0), (b1, t1) in zip(entries, entries[1:]):
                    if b0[4] == b1[4]:
                        assert order[t0.tobytes()] <= order[t1.tobytes()], (what, key)
    return kinds, (pairs, nodes, ls_tris, leaf_pairs)

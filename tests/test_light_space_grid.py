"""Light-space shadow grids (ft_flat.h, grid; option light_space_shadows = 2): every triangle is listed in every cell its rectangle
overlaps, by the float cell function the device uses, each cell's entries come by w_max descending, the caps hold, degenerate directions
and option 1 build none, and on the device the grid changes no bit of any frame or counter against the tree and the BVH."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import functracer_amd as ft
from tests.helpers import ROOT, scene_path
from tests.test_light_space_shadows import NONE, bunny_tris, built, camera_at, light_space, mesh_scene

ENTRIES_PER_TRI, MAX_CELL = 16, 256


def grid_of(rec):
    """(cells word offset, s, n_u, n_v) of a pair record; n_u = 0: the pair has no grid."""
    w = rec[14:16].view(np.uint32)
    return int(w[1]), float(w[2:3].view(np.float32)[0]), int(w[3]) & 0xFFFF, int(w[3]) >> 16


def f32_round(x):
    """An exact rational rounded to the nearest float32, ties to even (normal range)."""
    if x == 0:
        return Fraction(0)
    e = math.floor(math.log2(abs(x)))
    while Fraction(2) ** e > abs(x):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = x / ulp
    n = math.floor(q)
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return n * ulp


def cell(x, s, n):
    """The device's clamp(floor(fmaf(x, s, 0.5f * n)), 0, n - 1), exactly."""
    f = math.floor(f32_round(Fraction(float(x)) * Fraction(float(s)) + Fraction(n, 2)))
    return min(max(f, 0), n - 1)


def grid_cells(rec, nodes, ls_tris):
    """{(i, j): [(box[5], record), ...]} of a pair's grid, in stored order."""
    at, s, nu, nv = grid_of(rec)
    words = nodes.reshape(-1)
    out = {}
    for j in range(nv):
        for i in range(nu):
            first, box, count, zero = (int(x) for x in words[at + 4 * (j * nu + i):at + 4 * (j * nu + i) + 4])
            assert zero == 0
            boxes = words[box:box + 5 * count].view(np.float32).reshape(count, 5)
            out[(i, j)] = [(boxes[k], ls_tris[first + k]) for k in range(count)]
    return out


def check_grid(rec, nodes, ls_tris, n_tris):
    at, s, nu, nv = grid_of(rec)
    assert nu >= 1 and nv >= 1 and nu * nv >= 2 and s > 0 and at % 4 == 0
    U, V, D, c = rec[0:3], rec[3:6], rec[6:9], rec[9:12]
    cells = grid_cells(rec, nodes, ls_tris)
    boxes, listed = {}, {}
    total = 0
    for key, entries in cells.items():
        assert len(entries) <= MAX_CELL
        w = [float(b[4]) for b, _ in entries]
        assert w == sorted(w, reverse=True), key
        total += len(entries)
        for b, t in entries:
            tk = t.tobytes()
            assert boxes.setdefault(tk, b.tobytes()) == b.tobytes()      # one box per triangle, whatever cell lists it
            per = listed.setdefault(tk, {})
            per[key] = per.get(key, 0) + 1
    # a mesh may hold one triangle several times: equal records are listed once each, so equally often in every cell that lists them
    copies = {tk: set(per.values()) for tk, per in listed.items()}
    assert all(len(c) == 1 for c in copies.values())
    assert sum(next(iter(c)) for c in copies.values()) == n_tris and total <= ENTRIES_PER_TRI * n_tris
    for tk, bb in boxes.items():
        b = np.frombuffer(bb, dtype=np.float32)
        t = np.frombuffer(tk, dtype=np.float64)
        v0 = t[0:3] - c
        for q in (v0, v0 + t[3:6], v0 + t[6:9]):                         # the box holds the triangle
            u, v, w = q @ U, q @ V, q @ D
            assert b[0] <= u <= b[1] and b[2] <= v <= b[3] and w <= b[4]
        want = {(i, j) for j in range(cell(b[2], s, nv), cell(b[3], s, nv) + 1) for i in range(cell(b[0], s, nu), cell(b[1], s, nu) + 1)}
        assert set(listed[tk]) == want                                     # every cell its rectangle overlaps, and no other
    return cells


def test_grid_lists_every_triangle_in_every_cell_it_overlaps():
    tris = bunny_tris()
    ctx = ft.Context(host_only=True)
    xf = [("scale", (8.0, 3.0, 5.0)), ("rotate", (1.0, 2.0, 3.0), 0.7)]
    mesh_scene(ctx, tris, [("dir", (-3, -2, 3)), ("point", (0, 5, 0)), ("dir", (0, -1, 0))], xf=xf)
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    recs = pairs[leaf_pairs[0]:leaf_pairs[0] + 3]
    assert grid_of(recs[1])[2] == 0                                        # a point light has neither tree nor grid
    want = {tuple(np.concatenate([t[0:3], t[3:6] - t[0:3], t[6:9] - t[0:3]]).tolist()) for t in tris}
    for l in (0, 2):
        cells = check_grid(recs[l], nodes, ls_tris, len(tris))
        occupied = [len(e) for e in cells.values() if e]
        assert 2.0 <= np.mean(occupied) <= 16.0                            # the resolution aims at a few entries per occupied cell
    assert {tuple(r.tolist()) for r in ls_tris} == want                    # bitwise copies of the mesh's own records
    ctx.close()


def test_headline_scene_gets_a_grid():
    ctx = ft.Context(host_only=True)
    ft.parse_scene_file(scene_path("bunny")).lower(ctx)
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    lit = [k for k in leaf_pairs if k != 0xFFFFFFFF]
    assert lit
    rec = pairs[lit[0]]
    assert int(rec[14:15].view(np.int32)[0]) >= 0
    check_grid(rec, nodes, ls_tris, 980)
    ctx.close()


def test_axis_aligned_lights_get_grids():
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, bunny_tris(), [("dir", (0, 0, 1)), ("dir", (1, 0, 0))])
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    for l in range(2):
        check_grid(pairs[leaf_pairs[0] + l], nodes, ls_tris, 980)
    ctx.close()


def test_degenerate_direction_gets_none():
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, bunny_tris(), [("dir", (0, 0, 0)), ("dir", (1, -1, 0))])
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    none, some = pairs[leaf_pairs[0]], pairs[leaf_pairs[0] + 1]
    assert int(none[14:15].view(np.int32)[0]) == NONE and grid_of(none)[2] == 0
    check_grid(some, nodes, ls_tris, 980)
    ctx.close()


def test_flat_mesh_edge_on_stays_within_the_caps():
    g = np.linspace(-1.0, 1.0, 9)
    quads = []
    for i in range(8):
        for j in range(8):
            a, b, c, d = (g[i], 0, g[j]), (g[i + 1], 0, g[j]), (g[i + 1], 0, g[j + 1]), (g[i], 0, g[j + 1])
            quads += [[*a, *b, *c], [*a, *c, *d]]
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, np.array(quads, dtype=np.float64), [("dir", (1, 0, 0)), ("dir", (1e-3, -1, 2e-3))])
    pairs, nodes, ls_tris, leaf_pairs = light_space(ctx)
    for l in range(2):
        rec = pairs[leaf_pairs[0] + l]
        if grid_of(rec)[2]:
            check_grid(rec, nodes, ls_tris, 128)
    ctx.close()


def test_option_values_pick_what_is_built():
    tris = bunny_tris()
    ctx = ft.Context(host_only=True)
    built_grid = {}
    for opt in (2, 1, -1, 0):
        ctx.set_option("light_space_shadows", opt)
        mesh_scene(ctx, tris, [("dir", (-3, -2, 3))])
        pairs, _, _, leaf_pairs = light_space(ctx)
        built_grid[opt] = None if leaf_pairs[0] == 0xFFFFFFFF else grid_of(pairs[leaf_pairs[0]])[2] > 0
    assert built_grid == {2: True, 1: False, -1: True, 0: None}            # any value but 0 / 1 means the grid, as the flag did
    ctx.close()


def test_default_builds_grids():
    ctx = ft.Context(host_only=True)
    mesh_scene(ctx, bunny_tris(), [("dir", (-3, -2, 3))])
    pairs, _, _, leaf_pairs = light_space(ctx)
    assert grid_of(pairs[leaf_pairs[0]])[2] > 0
    ctx.close()


# ---- on the device: the grid changes no bit ----------------------------------------------------------------------------------------

def render_three(ctx, lower, cam, w, h, spp, jitter=None, tiles=None):
    jit = ft.jitter_pattern(spp) if jitter is None else jitter
    out = []
    for opt in (0, 1, 2):
        ctx.set_option("light_space_shadows", opt)
        lower(ctx)
        img, st = ctx.render(cam, w, h, spp, jit, tiles=tiles)
        out.append((img, {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}))
    ctx.set_option("light_space_shadows", 2)
    for img, st in out[1:]:
        assert np.array_equal(out[0][0], img), f"frames differ on {np.count_nonzero(np.any(out[0][0] != img, axis=2))} pixels"
        assert st == out[0][1]
    return out[0]


def flat_tiles(n=8, half=1.0):
    g = np.linspace(-half, half, n + 1)
    quads = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = (g[i], 0, g[j]), (g[i + 1], 0, g[j]), (g[i + 1], 0, g[j + 1]), (g[i], 0, g[j + 1])
            quads += [[*a, *b, *c], [*a, *c, *d]]
    return np.array(quads, dtype=np.float64)


@pytest.mark.gpu
def test_headline_scene_identical(hip):
    p = ft.parse_scene_file(scene_path("bunny"))
    _, st = render_three(hip, p.lower, p.camera, 480, 270, 4)
    assert st["rays_shadow"] > 0


@pytest.mark.gpu
def test_headline_scene_far_and_coarse_identical(hip):
    """Waves far apart in the light's frame: most cover several cells, and the wide ones take the tree."""
    p = ft.parse_scene_file(scene_path("bunny"))
    render_three(hip, p.lower, p.camera, 96, 54, 2)


@pytest.mark.gpu
def test_scaled_rotated_bunny_identical(hip):
    xf = [("scale", (8.0, 3.0, 5.0)), ("rotate", (1.0, 2.0, 3.0), 0.7)]
    render_three(hip, built(bunny_tris(), [("dir", (-3, -2, 3))], xf=xf), camera_at((0, 2, -4), (0, 0, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_axis_light_identical(hip):
    xf = [("scale", (8.0, 8.0, 8.0))]
    render_three(hip, built(bunny_tris(), [("dir", (0, -1, 0))], xf=xf), camera_at((0, 2, -3), (0, 0.5, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_grazing_light_on_flat_mesh_identical(hip):
    bunny = lambda ctx: [ctx.material(ctx.transform([("scale", (4.0, 4.0, 4.0))], ctx.bsp_mesh(0, bunny_tris())), colour=(1, 1, 1))]
    render_three(hip, built(flat_tiles(), [("dir", (1, 0, 0)), ("dir", (0, 0, -1))], xf=[("scale", (3.0, 3.0, 3.0))], extra=bunny),
                 camera_at((0, 3, -5), (0, 0, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_hit_points_straddle_cell_borders_identical(hip):
    """A tiled floor, finer than the grid, under a light a hair off its normal: the grid's axes run almost along the tile edges, and
    the bunny's shadow and the floor's hit points fall on both sides of cell borders across the frame."""
    bunny = lambda ctx: [ctx.material(ctx.transform([("scale", (4.0, 4.0, 4.0)), ("translate", (0.0, 0.3, 0.0))],
                                                    ctx.bsp_mesh(0, bunny_tris())), colour=(1, 1, 1))]
    lights = [("dir", (1e-4, -1.0, 3e-5)), ("dir", (0.0, -1.0, 1e-6))]
    render_three(hip, built(flat_tiles(24, 1.0), lights, xf=[("scale", (3.0, 3.0, 3.0))], extra=bunny),
                 camera_at((0.3, 4, -3), (0, 0, 0)), 320, 240, 4)


@pytest.mark.gpu
def test_two_directional_and_a_point_light_identical(hip):
    xf = [("scale", (8.0, 8.0, 8.0)), ("rotate", (0.0, 1.0, 0.0), math.pi)]
    render_three(hip, built(bunny_tris(), [("dir", (-3, -2, 3)), ("point", (1, 4, -2)), ("dir", (2, -1, 1))], xf=xf),
                 camera_at((0, 2, -2), (0, 0, 3)), 256, 256, 2)


@pytest.mark.gpu
def test_mesh_beside_csg_identical(hip):
    def csg(ctx):
        a = ctx.translate((1.5, 0.5, 0.0), ctx.primitive(ft.SPHERE))
        b = ctx.translate((1.9, 0.5, 0.0), ctx.primitive(ft.CUBE))
        return [ctx.material(ctx.subtract(a, b), colour=(0.3, 0.6, 0.9)), ctx.material(ctx.primitive(ft.PLANE), colour=(0.5, 0.5, 0.5))]
    render_three(hip, built(bunny_tris(), [("dir", (-3, -2, 3))], xf=[("scale", (8.0, 8.0, 8.0))], extra=csg),
                 camera_at((0, 2, -4), (0.5, 0.5, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_large_mesh_device_built_identical(hip):
    path = os.path.join(ROOT, "scenes", "meshes", "bunny_synth_full.ply")
    with open(path) as f:
        tris = ft.parse_ply(f.read())
    assert len(tris) >= 4096
    render_three(hip, built(tris, [("dir", (-3, -2, 3))], xf=[("scale", (8.0, 8.0, 8.0))]), camera_at((0, 2, -2), (0, 0.5, 0)), 256, 256, 2)


@pytest.mark.gpu
def test_recommit_after_light_change_identical(hip):
    xf = [("scale", (8.0, 8.0, 8.0))]
    cam = camera_at((0, 2, -2), (0, 0.5, 0))
    a, _ = render_three(hip, built(bunny_tris(), [("dir", (-3, -2, 3))], xf=xf), cam, 192, 192, 2)
    b, _ = render_three(hip, built(bunny_tris(), [("dir", (3, -2, -1))], xf=xf), cam, 192, 192, 2)
    assert not np.array_equal(a, b)                                        # the shadows moved

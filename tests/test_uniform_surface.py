"""One-leaf batches of k_primary (option uniform_surface): when every hit lane of a coherent wave hit the same leaf, the leaf's head,
matrices and material come through scalar loads of that one leaf index, the shaders skip what no lane of the wave can use, and a batch
whose candidate list is empty stores Colour.Zero without generating its rays.  Every value that reaches a pixel is computed by the same
expression either way, so no bit of any frame or counter may move with the option; each frame is also held against the CPU oracle."""
import math
import os

import numpy as np
import pytest

import functracer_amd as ft
from functracer_amd import _capi
from oracle import ft_oracle_py as O
from tests import bvh_tools as BT
from tests import helpers as H

DIR = ("dir", (-3, -2, 3))
GROUPINGS = [(32, 32, 16), (64, 32, 4), (32, 32, 3)]       # grouped numbering at 16 and at 4 samples a wave; plain numbering


def counters(st):
    return {k: v for k, v in st.items() if not k.endswith("_ms") and "time" not in k}


def camera_at(o, look):
    return ft.make_camera(o, look, (0, 1, 0), math.radians(60), 1.0)


def wavy(n, half=1.0, amp=0.15):
    """A height field over [-half, half]^2 in the xz plane, 2 n^2 triangles, normals up."""
    g = np.linspace(-half, half, n + 1)
    hgt = lambda x, z: amp * math.sin(3.0 * x) * math.cos(2.0 * z)
    quads = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = [(x, hgt(x, z), z) for x, z in ((g[i], g[j]), (g[i + 1], g[j]), (g[i + 1], g[j + 1]), (g[i], g[j + 1]))]
            quads += [[*a, *c, *b], [*a, *d, *c]]
    return np.array(quads, dtype=np.float64)


def bunny_tris():
    with open(os.path.join(H.ROOT, "scenes", "meshes", "bunny_synth_res4.ply")) as f:
        return ft.parse_ply(f.read())


def add_lights(b, lights):
    for kind, v in lights:
        if kind == "dir":
            b.add_directional(v, (1, 1, 1))
        else:
            b.add_positional(v, (1, 0.01, 0.02), (1, 1, 1))


def scene_of(items, lights=(DIR,)):
    """lower(builder) for a scene whose top-level items `items(builder)` lists."""
    def lower(b):
        b.clear()
        b.set_objects(b.group(items(b)))
        add_lights(b, lights)
        b.commit()
    return lower


def both_and_oracle(ctx, lower, cam, w, h, spp, max_depth=ft.MAX_DEPTH, lists=1):
    """The frame with uniform_surface = 0 and = 1: equal bit for bit, every counter too, and within the parity tolerance of the oracle's."""
    jit = ft.jitter_pattern(spp)
    lower(ctx)
    out = []
    try:
        ctx.set_option("primary_block_lists", lists)
        for opt in (1, 0, 1):                                        # (the first frame of a scene launches every reflection level, its successors as many
            ctx.set_option("uniform_surface", opt)                   # as their predecessor used: n_launches is compared between the second and the third)
            img, st = ctx.render(cam, w, h, spp, jit, max_depth=max_depth)
            out.append((img, counters(st)))
        assert np.array_equal(out[0][0], out[2][0])
        out = out[1:]
    finally:
        ctx.set_option("uniform_surface", 1)
        ctx.set_option("primary_block_lists", 1)
    (a, sa), (b, sb) = out
    assert np.array_equal(a, b), f"frames differ on {np.count_nonzero(np.any(a != b, axis=2))} pixels"
    assert sa == sb
    orc = O.Oracle()
    lower(orc)
    want, _ = orc.render(cam, w, h, spp, jit, max_depth=max_depth)
    H.assert_frames_match(b, want, what=f"{w}x{h}x{spp}")
    return b, sb


def leaf_planes(ctx, cam, w, h, spp):
    """ft_render_aov's leaf plane of every sample of the frame: [spp, h, w]."""
    jit = ft.jitter_pattern(spp)
    return np.stack([ctx.render_aov(cam, w, h, spp, jit, sample=s, channels=["leaf"])["leaf"] for s in range(spp)])


def blocks_of(leaf):
    """[spp, h, w] -> [h / 8, w / 8, spp * 64]: the samples of each 8x8 block."""
    s, h, w = leaf.shape
    return leaf.reshape(s, h // 8, 8, w // 8, 8).transpose(1, 3, 0, 2, 4).reshape(h // 8, w // 8, s * 64)


_B = BT.blob(64)                                                     # the catalogue's blob(64), each triangle grown five-fold about its
BLOB = _B.mean(axis=1, keepdims=True) + 5.0 * (_B - _B.mean(axis=1, keepdims=True))   # centroid so that the mesh fills a small frame
BLOB_CAM = BT.camera((0.0, 0.0, 0.0), 1.5)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", GROUPINGS)
@pytest.mark.parametrize("xf", [None, [("scale", (1.3, 0.8, 1.1)), ("rotate", (1.0, 2.0, 3.0), 0.7)]], ids=["bare", "xform"])
def test_one_bare_mesh(hip, xf, w, h, spp):
    def items(b):
        node = b.bsp_mesh(0, BLOB.reshape(-1, 9))
        return [b.material(b.transform(xf, node) if xf else node, colour=(0.8, 0.7, 0.6))]
    frame, st = both_and_oracle(hip, scene_of(items, [DIR, ("point", (1, 4, -2))]), BLOB_CAM, w, h, spp)
    assert st["hits_primary"] > 0 and frame.max() > 0.05


def two_sheets(b):
    """Two height fields with different materials whose seam runs slanted across the frame (the left one overlaps the right one, which
    lies a little lower, so no ray passes between them): no 8x8 block the seam crosses is one leaf."""
    left = b.transform([("scale", (1.5, 1.0, 3.0)), ("rotate", (0, 1, 0), 0.29), ("translate", (-1.3, 0.0, 0.0))], b.bsp_mesh(0, wavy(3).reshape(-1, 9)))
    right = b.transform([("scale", (1.5, 1.0, 3.0)), ("rotate", (0, 1, 0), 0.29), ("translate", (1.3, -0.3, 0.0))], b.bsp_mesh(0, wavy(3).reshape(-1, 9)))
    return [b.material(left, colour=(0.9, 0.3, 0.2)), b.material(right, colour=(0.2, 0.4, 0.9), shineyness=3.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", GROUPINGS)
def test_wave_straddles_two_leaves(hip, w, h, spp):
    cam = camera_at((0.1, 3.0, -2.5), (0, 0, 0))
    frame, st = both_and_oracle(hip, scene_of(two_sheets), cam, w, h, spp)
    # by construction both paths ran: a strip of four pixels of one row - part of every wave's share of its block, whatever the grouping -
    # sees both leaves, and another block sees one leaf with every sample of every pixel
    leaf = leaf_planes(hip, cam, w, h, spp)
    strips = leaf[0].reshape(h, w // 4, 4)
    split = (strips.min(axis=2) >= 0) & (strips.min(axis=2) != strips.max(axis=2))
    blocks = blocks_of(leaf)
    whole = (blocks.min(axis=2) >= 0) & (blocks.min(axis=2) == blocks.max(axis=2))
    assert split.any() and whole.any(), (int(split.sum()), int(whole.sum()))
    assert st["hits_primary"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", GROUPINGS)
def test_dull_mesh_beside_a_shiny_sphere(hip, w, h, spp):
    """shineyness 0 and 8 in one wave: a lane that wants the specular term gets it whatever its neighbours want."""
    def items(b):
        mesh = b.transform([("scale", (2.0, 1.0, 2.0))], b.bsp_mesh(0, wavy(3).reshape(-1, 9)))
        ball = b.transform([("scale", (0.7, 0.7, 0.7)), ("translate", (0.4, 0.5, 0.0))], b.primitive(ft.SPHERE))
        return [b.material(mesh, colour=(0.8, 0.7, 0.6)), b.material(ball, colour=(0.3, 0.8, 0.4), shineyness=8.0)]
    cam = camera_at((0.3, 2.0, -2.5), (0.2, 0.3, 0))
    frame, st = both_and_oracle(hip, scene_of(items, [("dir", (1, -2, 2))]), cam, w, h, spp)
    leaf = leaf_planes(hip, cam, w, h, 1)[0].reshape(h, w // 4, 4)
    assert ((leaf.min(axis=2) >= 0) & (leaf.min(axis=2) != leaf.max(axis=2))).any()      # mesh and sphere in one strip of four pixels
    assert st["hits_primary"] > 0 and frame.max() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", GROUPINGS)
def test_reflective_mesh_at_depth_two(hip, w, h, spp):
    def items(b):
        mesh = b.transform([("scale", (2.0, 1.0, 2.0))], b.bsp_mesh(0, wavy(3).reshape(-1, 9)))
        ball = b.transform([("scale", (0.5, 0.5, 0.5)), ("translate", (0.0, 0.9, 0.3))], b.primitive(ft.SPHERE))
        return [b.material(mesh, colour=(0.8, 0.7, 0.6), reflectance=0.5), b.material(ball, colour=(0.9, 0.2, 0.2))]
    _, st = both_and_oracle(hip, scene_of(items), camera_at((0.3, 2.0, -2.5), (0, 0.3, 0)), w, h, spp, max_depth=2)
    assert st["rays_reflect"] > 0 and st["rays_reflect_primary"] > 0


HOLE_C, HOLE_R = (0.0, 0.5, 0.0), 0.45


def carved_beside_a_mesh(b):
    """A cube with a bowl a sphere leaves in its top (subtract flips B's normals: every hit on the sphere's leaf carries ID_FLIP), and a
    mesh beside it, so that the frame runs the mesh kernel - the one the one-leaf path is compiled into."""
    hole = b.transform([("scale", (HOLE_R,) * 3), ("translate", HOLE_C)], b.primitive(ft.SPHERE))
    carved = b.material(b.subtract(b.primitive(ft.CUBE), hole), colour=(0.7, 0.7, 0.9), shineyness=2.0)
    sheet = b.transform([("scale", (0.5, 1.0, 0.5)), ("translate", (1.1, 0.0, 0.0))], b.bsp_mesh(0, wavy(3).reshape(-1, 9)))
    return [carved, b.material(sheet, colour=(0.8, 0.7, 0.6))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", GROUPINGS)
def test_flipped_hits_on_the_one_leaf_path(hip, w, h, spp):
    """ID_FLIP through the one-leaf path: whole 8x8 blocks - so whole waves, whatever the grouping - lie on the bowl's leaf, whose every
    hit is flipped, in a scene with a mesh.  (One leaf's first hits cannot mix flipped and unflipped lanes: a CSG fold decides the flip from
    the side and the inside flags, which are the same for every visible hit of a leaf.  The flattener sets LF_FLIP on no leaf.)"""
    cam = camera_at((0.2, 1.3, -0.3), (0.1, 0.3, 0.0))
    _, st = both_and_oracle(hip, scene_of(carved_beside_a_mesh, [("dir", (1, -2, 2))]), cam, w, h, spp)
    assert st["hits_primary"] > 0
    jit = ft.jitter_pattern(spp)
    aov = [hip.render_aov(cam, w, h, spp, jit, sample=s, channels=["leaf", "p", "n"]) for s in range(spp)]
    leaf, p, n = (np.stack([a[k] for a in aov]) for k in ("leaf", "p", "n"))
    rel = p - np.array(HOLE_C)
    on_bowl = (leaf >= 0) & (np.abs(np.linalg.norm(rel, axis=-1) - HOLE_R) < 1e-6)
    assert on_bowl.any()
    bowl_leaf = np.unique(leaf[on_bowl])
    assert bowl_leaf.size == 1, bowl_leaf
    of_leaf = leaf == bowl_leaf[0]
    assert np.array_equal(of_leaf, on_bowl) and (np.einsum("...k,...k->...", n, rel)[of_leaf] < 0.0).all()   # every hit of the leaf: the normal points into the bowl
    blocks = blocks_of(leaf)
    whole = (blocks.min(axis=2) == bowl_leaf[0]) & (blocks.max(axis=2) == bowl_leaf[0])
    strips = leaf[0].reshape(h, w // 4, 4)
    rim = (strips.min(axis=2) >= 0) & (strips == bowl_leaf[0]).any(axis=2) & (strips != bowl_leaf[0]).any(axis=2)   # bowl and cube top in one strip: per lane
    assert whole.any() and rim.any(), (int(whole.sum()), int(rim.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", GROUPINGS)
def test_mesh_seen_from_inside(hip, w, h, spp):
    """The camera and a point light inside a closed mesh wound inside out, so that its normals face them and the walls are lit."""
    def bunny(b):
        return [b.material(b.transform([("scale", (8.0, 8.0, 8.0))], b.bsp_mesh(0, bunny_tris()[:, [0, 1, 2, 6, 7, 8, 3, 4, 5]])), colour=(0.8, 0.7, 0.6))]
    tris = bunny_tris().reshape(-1, 3, 3) * 8.0
    inside = tuple(0.5 * (tris.reshape(-1, 3).min(axis=0) + tris.reshape(-1, 3).max(axis=0)))
    lower = scene_of(bunny, [("point", inside)])
    frame, st = both_and_oracle(hip, lower, camera_at(inside, (inside[0] + 1.0, inside[1], inside[2] + 0.3)), w, h, spp)
    assert st["hits_primary"] > 0 and frame.max() > 0.05


def shell(n=64, seed=5):
    """n small triangles spread over a sphere of radius 2: the boxes over any four of them hold far more sky than triangle."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 1, 3))
    c = 2.0 * c / np.linalg.norm(c, axis=2, keepdims=True)
    return (c + rng.normal(size=(n, 3, 3)) * 0.04).reshape(-1, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [4, 16])
@pytest.mark.parametrize("ground", [False, True], ids=["alone", "with_ground"])
def test_block_with_an_empty_candidate_list(hip, ground, spp):
    """A block the coarse boxes keep active but no triangle's rectangle overlaps: its batches store Colour.Zero without a ray when the
    mesh is the scene's only item, and trace like any other when a ground (a wide disc) lies below it."""
    def items(b):
        out = [b.material(b.bsp_mesh(0, shell()), colour=(0.8, 0.7, 0.6))]
        if ground:
            # (a disc of radius 40, not the infinite plane: a frame over an unbounded item is not classified and carries no lists)
            out.append(b.material(b.transform([("scale", (40.0, 1.0, 40.0)), ("translate", (0.0, -2.5, 0.0))], b.primitive(ft.CIRCLE)), colour=(0.3, 0.6, 0.3)))
        return out
    cam = camera_at((0.5, 1.0, -6.0), (0, 0, 0))
    w, h = 64, 32
    frame, st = both_and_oracle(hip, scene_of(items), cam, w, h, spp)
    L = hip.block_lists()                                            # of the last frame rendered: uniform_surface = 1, lists on
    listed = L["heads"] != _capi.LIST_NONE
    assert L["leaf"] >= 0 and (listed & ((L["heads"] & 127) == 0)).any(), "no active block carries an empty list"
    assert (listed & ((L["heads"] & 127) != 0)).any() and st["hits_primary"] > 0
    if ground:
        blocks = blocks_of(leaf_planes(hip, cam, w, h, spp))
        empty_pos = L["pos_block"][listed & ((L["heads"] & 127) == 0)]
        assert any((blocks[p // (w // 8), p % (w // 8)] >= 0).any() for p in empty_pos), "no empty-list block sees the ground"
    # the same frame without the lists: nothing depends on them
    off, st_off = both_and_oracle(hip, scene_of(items), cam, w, h, spp, lists=0)
    assert np.array_equal(off, frame) and st_off == st


@pytest.mark.gpu
def test_headline_scene(hip):
    p = ft.parse_scene_file(H.scene_path("bunny"))
    _, st = both_and_oracle(hip, p.lower, p.camera, 64, 36, 16)
    assert st["rays_shadow"] > 0

"""The numpy replay of option "light_space_retree" (include/functracer_hip.h "moving lights"): what the device leaves in a
retreed pair's block of nodes and in its run of leaf records, word for word, from the mesh's list-order records, the pair record and R.

  keys      k_ls_keys: the (u, v) rectangle of a record as grow_by_tri projects it, in float64 and unfused (numpy fuses nothing), its
            centre, 16 bits per axis over [-R, R], interleaved with u in the even bits
  order     np.argsort(kind="stable") of the keys: what rocprim's radix sort of (key, list index) leaves
  topology  the host generator restated (ft_ls_topology.h): a function of n, the first leaf record and the first node alone
  boxes     k_ls_refit over that topology: leaf children from their records, node children from the union of the child's boxes, rounded
            outward through f_down / f_up
  cost      the 2-D surface-area cost the CPU tests compare a refit tree and a retreed one by"""
import numpy as np

NODE_WORDS = 24
LEAF = 4                                                            # LsBuilder::kLeafTris
EMPTY = -(1 << 31)
NAN_WORD = 0x7FC00000


# ---------------------------------------------------------------------------------------------------------------- the topology
def node_count(n):
    """N(n) in closed form: the binary node at depth d holds n >> d positions or one more, n mod 2^d of them the larger; a 4-wide node
    stands at every even depth where it holds more than four."""
    total, d = 0, 0
    while n > LEAF and (n >> d) >= LEAF:
        q, r = n >> d, n & ((1 << d) - 1)
        total += (1 << d) if q > LEAF else r
        d += 2
    return total


def topology(n, ls_first, first_node):
    """(child words [N, 4] int32, order [N] uint32, levels [k, 2] uint32: offset into order and count, deepest level first)."""
    assert n > LEAF
    ranges, child = [(0, n, 0)], []
    k = 0
    while k < len(ranges):
        lo, hi, level = ranges[k]
        k += 1
        words = [EMPTY] * 4
        mid = lo + (hi - lo) // 2
        for h, (a, b) in enumerate(((lo, mid), (mid, hi))):
            kids = [(a, b)] if b - a <= LEAF else [(a, a + (b - a) // 2), (a + (b - a) // 2, b)]
            for s, (x, y) in enumerate(kids):
                if y - x <= LEAF:
                    words[2 * h + s] = ~((ls_first + x) << 3 | (y - x))
                else:
                    words[2 * h + s] = first_node + len(ranges)
                    ranges.append((x, y, level + 1))
        child.append(words)
    depth = ranges[-1][2] + 1
    by_level = [[first_node + i for i, r in enumerate(ranges) if r[2] == d] for d in range(depth)]
    order, levels = [], []
    for d in reversed(range(depth)):
        levels.append((len(order), len(by_level[d])))
        order += by_level[d]
    return np.array(child, dtype=np.int32), np.array(order, dtype=np.uint32), np.array(levels, dtype=np.uint32).reshape(-1, 2)


def as_nodes(child, first_node):
    """The child words as a node array indexed like ls_nodes (rows below first_node stay empty), every box NaN: what the walkers of
    tests/shadow_tools.py and check_tree read."""
    nodes = np.full((first_node + len(child), NODE_WORDS), NAN_WORD, dtype=np.uint32)
    nodes[:, 20:24] = np.uint32(1 << 31)
    nodes[first_node:, 20:24] = child.view(np.uint32)
    return nodes


# ---------------------------------------------------------------------------------------------------------------- keys and order
def project(recs, frame):
    """(pu, pv, pw), each [n, 3]: the three vertices of every record (v0, e1, e2) in the frame (U, V, D, c), as grow_by_tri sums them."""
    U, V, D, c = frame
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 9)
    base = recs[:, 0:3] - c
    p = np.stack([base + 0.0, base + recs[:, 3:6], base + recs[:, 6:9]], axis=1)   # [n, vertex, xyz]

    def dot(a):
        return (p[:, :, 0] * a[0] + p[:, :, 1] * a[1]) + p[:, :, 2] * a[2]
    return dot(U), dot(V), dot(D)


def _spread16(v):
    v = v.astype(np.uint32) & np.uint32(0xFFFF)
    for shift, mask in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        v = (v | (v << np.uint32(shift))) & np.uint32(mask)
    return v


def keys(recs, frame, R):
    pu, pv, _ = project(recs, frame)
    out = []
    with np.errstate(all="ignore"):
        g = np.float64(32768.0) / np.float64(R)
        for p in (pu, pv):
            centre = 0.5 * (p.min(axis=1) + p.max(axis=1))
            cell = np.fmin(65535.0, np.fmax(0.0, np.floor((centre + R) * g)))   # fmin / fmax pass over a NaN
            out.append(_spread16(cell.astype(np.int64)))
    return out[0] | (out[1] << np.uint32(1))


def sorted_order(recs, frame, R):
    """perm: position i of the pair's leaf records copies list-order triangle perm[i]."""
    return np.argsort(keys(recs, frame, R), kind="stable")


def extent(recs, c):
    """R: the largest L1 distance of a vertex from the centre."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 9)
    base = recs[:, 0:3] - c
    p = np.stack([base, base + recs[:, 3:6], base + recs[:, 6:9]], axis=1)
    return float(np.abs(p).sum(axis=2).max())


# ---------------------------------------------------------------------------------------------------------------- boxes
def f_down(v):
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def f_up(v):
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def boxes(child, first_node, order, leaf_recs, ls_first, frame, pad):
    """k_ls_refit over a tree: [N, 4, 5] float32, NaN in the empty slots.  child: [N, 4] int32 of the nodes first_node ..; order: those
    nodes deepest level first; leaf_recs: the records the leaf words index, leaf_recs[0] being record ls_first of ls_tris."""
    pu, pv, pw = project(leaf_recs, frame)
    lo_u, hi_u, lo_v, hi_v, w = pu.min(axis=1), pu.max(axis=1), pv.min(axis=1), pv.max(axis=1), pw.max(axis=1)
    out = np.full((len(child), 4, 5), np.nan, dtype=np.float32)
    for node in order:
        k = int(node) - first_node
        for s in range(4):
            ch = int(child[k, s])
            if ch == EMPTY:
                continue
            if ch >= 0:
                b = out[ch - first_node]
                out[k, s] = (np.fmin.reduce(b[:, 0]), np.fmax.reduce(b[:, 1]), np.fmin.reduce(b[:, 2]), np.fmax.reduce(b[:, 3]), np.fmax.reduce(b[:, 4]))
                continue
            a = ((~ch) >> 3) - ls_first
            z = a + ((~ch) & 7)
            out[k, s] = (f_down(lo_u[a:z].min() - pad), f_up(hi_u[a:z].max() + pad), f_down(lo_v[a:z].min() - pad), f_up(hi_v[a:z].max() + pad),
                         f_up(w[a:z].max() + pad))
    return out


def levels_of(child, first_node, root):
    """The nodes of any tree deepest level first (the order boxes() needs), from its child words."""
    levels, level = [], [root]
    while level:
        levels.append(level)
        level = [int(c) for n in level for c in child[n - first_node] if c >= 0]
    return [n for lv in reversed(levels) for n in lv]


def cost(child, bx, first_node, root):
    """sum over all child boxes of the tree under `root` of area x (1 for a node child, the count for a leaf child) / the area of the union
    of the root's boxes."""
    total = 0.0
    for n in levels_of(child, first_node, root):
        k = n - first_node
        for s in range(4):
            ch = int(child[k, s])
            if ch == EMPTY:
                continue
            b = bx[k, s].astype(np.float64)
            total += (b[1] - b[0]) * (b[3] - b[2]) * (1 if ch >= 0 else (~ch) & 7)
    r = bx[root - first_node].astype(np.float64)
    area = (np.nanmax(r[:, 1]) - np.nanmin(r[:, 0])) * (np.nanmax(r[:, 3]) - np.nanmin(r[:, 2]))
    return total / area


def frame_of(rec):
    return rec[0:3], rec[3:6], rec[6:9], rec[9:12]


def pad_of(R):
    return 1e-7 * R + 1e-30


def replay(list_recs, first_tri, ls_first, first_node, rec, R):
    """What a retree of a pair leaves: (perm, child, order, levels, boxes) for the mesh's list-order records, the pair record and R."""
    frame = frame_of(rec)
    perm = sorted_order(list_recs, frame, R)
    child, order, levels = topology(len(perm), ls_first, first_node)
    bx = boxes(child, first_node, order, np.asarray(list_recs).reshape(-1, 9)[perm], ls_first, frame, pad_of(R))
    return perm, child, order, levels, bx


def height_field(quads, amplitude=8.0):
    """quads x quads unit quads over the (x, z) plane, two triangles each, y displaced by a fixed integer hash of the grid point."""
    i, j = np.meshgrid(np.arange(quads + 1, dtype=np.uint64), np.arange(quads + 1, dtype=np.uint64), indexing="ij")
    h = (i * np.uint64(73856093)) ^ (j * np.uint64(19349663))
    h = (h * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    y = amplitude * ((h >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.float64) / 65535.0
    p = np.stack([i.astype(np.float64), y, j.astype(np.float64)], axis=2)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]
    return np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([a, c, d], axis=2).reshape(-1, 3, 3)])


def records(tris):
    """The records (v0, e1, e2) of triangles given by their vertices, as the flattener writes them."""
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    return np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], axis=1)

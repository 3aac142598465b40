"""A numpy replay of k_refit_cost (ft_refit.hip) over what Context.mesh_trees() reads back, for tests/test_refit_rebuild.py.

The kernel visits every node SLOT of the mesh's range and decides by real_node() which of them are nodes of the tree; the replay WALKS the
tree from its root.  The two agree only when the range holds nothing but the tree - a slot the last build left behind is counted by the
kernel and never reached by the walk."""
import math

import numpy as np


def half_area(lo, hi):
    d = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    return float(d[0] * d[1] + d[1] * d[2] + d[2] * d[0])


def tree_cost(T, mesh=0):
    """(sum over the inner nodes of A(stored box) + sum over the leaves of n_tris x A(exact bound of the leaf's records)) / A(root's stored
    box), summed exactly (math.fsum); 0.0 when the root's area is 0 or not finite."""
    nodes, leaves, tris = T["nodes"], T["bsp_leaves"], T["tris"]
    bvh_root = int(T["meshes"][mesh, 1])
    assert int(T["meshes"][mesh, 0]) < 0 and bvh_root >= 0, "the mesh has no BVH"
    terms, stack, seen = [], [bvh_root], 0
    while stack:
        r = stack.pop()
        seen += 1
        assert seen <= 4 * tris.shape[0] + 4, "the tree does not end"
        if r >= 0:
            terms.append(half_area(nodes["bmin"][r], nodes["bmax"][r]))
            stack.extend([int(nodes["right"][r]), int(nodes["left"][r])])
            continue
        f, c = (int(x) for x in leaves[~r])
        t = tris[f:f + c]
        v = np.stack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]], axis=1).reshape(-1, 3)   # as the hit test sees them
        terms.append(c * half_area(v.min(axis=0), v.max(axis=0)))
    root = half_area(nodes["bmin"][bvh_root], nodes["bmax"][bvh_root])
    return math.fsum(terms) / root if root > 0.0 and math.isfinite(root) else 0.0

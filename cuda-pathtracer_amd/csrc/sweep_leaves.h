/* sweep_leaves.h — the sweep's third image: the LEAVES of the tree alone, in pre-order, for the walk that slab-tests no interior
 * node (traversal.h: sweep_leaves_walk), free of HIP so that a plain C compiler can check the preparation and the verdict on the
 * host (tests/test_sweep_leaves_host.py) before a kernel walks it.
 *
 * One leaf is 64 bytes, the three axis groups as in the near/far records (sweep_near_far.h):
 *
 *   bytes  0..15   lo.x  hi.x  hi.x  lo.x        8 bytes at  0 + (1 / d.x < 0 ? 8 : 0)  ->  (near, far) along x
 *   bytes 16..31   lo.y  hi.y  hi.y  lo.y        8 bytes at 16 + (1 / d.y < 0 ? 8 : 0)
 *   bytes 32..47   lo.z  hi.z  hi.z  lo.z        8 bytes at 32 + (1 / d.z < 0 ? 8 : 0)
 *   bytes 48..63   rec   count rec   count
 *
 * rec is the LDS address of the leaf's first primitive record (prims_at + 16 * prim_stride * first slot), count its number of
 * primitives (> 0).  The pair stands twice so that a lane reads it at its x address + 48, whichever of the two x offsets it holds:
 * the walk then needs no address beside the three of the slab test.  Every float keeps its bits.
 *
 * The image stands behind the materials: [near/far nodes | primitives | frame block | materials | leaves]; no other offset moves
 * and the full node image stays where it is, for the waves that walk every node.
 *
 * The leaf-only walk is the reference's only over a tree whose boxes contain their children's, plane by plane, with every plane
 * finite (the proof is traversal.h's).  The builder gives that by construction; ptmi_sweep_leaves_verdict checks it, and the
 * links with it, on the node array itself, so the walk depends on no property of the builder.
 */
#ifndef PTMI_SWEEP_LEAVES_H
#define PTMI_SWEEP_LEAVES_H

#include "sweep_near_far.h"

#define PTMI_SWEEP_LEAF_VECS 4
#define PTMI_SWEEP_LEAF_BYTES (PTMI_SWEEP_LEAF_VECS * PTMI_SWEEP_VEC_BYTES)
#define PTMI_SWEEP_LEAF_LINK 48                       /* byte offset of (rec, count); (rec, count) again at + 8 */

/* [near/far nodes | primitives | frame block | materials | n_leaves leaf records] */
PTMI_HD size_t ptmi_sweep_leaves_lds_vecs(int n_nodes, int prim_stride, int n_prims, int n_leaves) {
    return ptmi_sweep_near_far_lds_vecs(n_nodes, prim_stride, n_prims) + PTMI_SWEEP_LEAF_VECS * (size_t)n_leaves;
}

PTMI_HD float ptmi_u2f(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
PTMI_HD int ptmi_is_leaf(const ptmi_vec_bits* nodes, int i) { return (int32_t)nodes[2 * i + 1].w < 0; }

PTMI_HD int ptmi_sweep_leaf_count(const ptmi_vec_bits* nodes, int n_nodes) {
    int i, n = 0;
    for (i = 0; i < n_nodes; i++) n += ptmi_is_leaf(nodes, i);
    return n;
}

/* Where the subtree of node j ends in pre-order, as the array itself says: a leaf ends behind itself, an interior node at its skip entry */
PTMI_HD int64_t ptmi_sweep_subtree_end(const ptmi_vec_bits* nodes, int j) {
    return ptmi_is_leaf(nodes, j) ? (int64_t)j + 1 : (int64_t)(int32_t)nodes[2 * j].w;
}

/* 1: the six planes of every node are finite, every interior node's planes bound those of its two children (lo <= lo, hi >= hi
 * per axis, as numbers: a NaN fails), the links are exactly pre-order's - the left child is the next record, the right child stands
 * where the left child's subtree ends, the skip entry where the right child's ends, the root's subtree ends at n_nodes (by induction
 * every skip entry is then the end of its node's subtree, so the leaves in array order are the leaves the links reach, in the
 * order they reach them) - and every leaf holds at least one of the n_prims slots.  0 otherwise: the walk then visits every node. */
PTMI_HD int ptmi_sweep_leaves_verdict(const ptmi_vec_bits* nodes, int n_nodes, int n_prims) {
    int i, c, a;
    if (n_nodes < 1 || ptmi_sweep_subtree_end(nodes, 0) != n_nodes) return 0;
    for (i = 0; i < n_nodes; i++) {
        const ptmi_vec_bits lo = nodes[2 * i], hi = nodes[2 * i + 1];
        const float plane[6] = {ptmi_u2f(lo.x), ptmi_u2f(lo.y), ptmi_u2f(lo.z), ptmi_u2f(hi.x), ptmi_u2f(hi.y), ptmi_u2f(hi.z)};
        for (a = 0; a < 6; a++)
            if (!(plane[a] - plane[a] == 0.0f)) return 0;                             /* inf or NaN */
        if ((int32_t)hi.w < 0) {                                                      /* leaf: first slot, -count */
            const int64_t first = (int64_t)(int32_t)lo.w, count = -(int64_t)(int32_t)hi.w;
            if (first < 0 || first + count > n_prims) return 0;
            continue;
        }
        {
            const int64_t right = (int64_t)(int32_t)hi.w, skip = (int64_t)(int32_t)lo.w;
            const int child[2] = {i + 1, (int)right};
            if (right <= i + 1 || right >= n_nodes || skip <= right || skip > n_nodes) return 0;
            if (ptmi_sweep_subtree_end(nodes, i + 1) != right || ptmi_sweep_subtree_end(nodes, (int)right) != skip) return 0;
            for (c = 0; c < 2; c++) {
                const ptmi_vec_bits clo = nodes[2 * child[c]], chi = nodes[2 * child[c] + 1];
                if (!(plane[0] <= ptmi_u2f(clo.x) && plane[1] <= ptmi_u2f(clo.y) && plane[2] <= ptmi_u2f(clo.z))) return 0;
                if (!(plane[3] >= ptmi_u2f(chi.x) && plane[4] >= ptmi_u2f(chi.y) && plane[5] >= ptmi_u2f(chi.z))) return 0;
            }
        }
    }
    return 1;
}

/* The leaf records, prepared from the scene's nodes: nodes first, first + step, ... (a workgroup calls it with its thread index
 * and size, the host with 0 and 1); a leaf's place is the number of leaves in front of it.  prims_at: the address the first
 * primitive record will stand at.  in and out must not overlap. */
PTMI_HD void ptmi_sweep_leaves_prepare(const ptmi_vec_bits* nodes, int n_nodes, int prim_stride, ptmi_vec_bits* out_leaves, uint32_t prims_at,
                                       int first, int step) {
    int i, j, at = 0, counted = 0;
    for (i = first; i < n_nodes; i += step) {
        const ptmi_vec_bits lo = nodes[2 * i], hi = nodes[2 * i + 1];
        if ((int32_t)hi.w >= 0) continue;
        for (j = counted; j < i; j++) at += ptmi_is_leaf(nodes, j);
        counted = i;
        {
            ptmi_vec_bits* o = out_leaves + (size_t)PTMI_SWEEP_LEAF_VECS * at;
            const ptmi_vec_bits x = {lo.x, hi.x, hi.x, lo.x}, y = {lo.y, hi.y, hi.y, lo.y}, z = {lo.z, hi.z, hi.z, lo.z};
            const uint32_t rec = prims_at + lo.w * (uint32_t)(prim_stride * PTMI_SWEEP_VEC_BYTES), count = 0u - hi.w;
            const ptmi_vec_bits w = {rec, count, rec, count};
            o[0] = x; o[1] = y; o[2] = z; o[3] = w;
        }
    }
}

#endif /* PTMI_SWEEP_LEAVES_H */

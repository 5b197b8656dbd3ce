/* sweep_near_far.h — the sweep's second node image: each axis of a node's box laid out so that a lane reads (near, far) for its
 * own ray by address, free of HIP so that a plain C compiler can check the preparation on the host
 * (tests/test_sweep_near_far_host.py) before a kernel walks it.
 *
 * Which of a box's two planes along an axis a ray meets first is decided by the sign of 1 / d along that axis, once for the whole
 * walk.  The slab test over the two-vector records (traversal.h: box_hit) subtracts lo first and swaps the two products per axis
 * and per node; here the lane reads the plane that belongs first into the first place.  One node is 64 bytes:
 *
 *   bytes  0..15   lo.x  hi.x  hi.x  lo.x        8 bytes at  0 + (1 / d.x < 0 ? 8 : 0)  ->  (near, far) along x
 *   bytes 16..31   lo.y  hi.y  hi.y  lo.y        8 bytes at 16 + (1 / d.y < 0 ? 8 : 0)
 *   bytes 32..47   lo.z  hi.z  hi.z  lo.z        8 bytes at 32 + (1 / d.z < 0 ? 8 : 0)
 *   bytes 48..63   w0    w1    0     0
 *
 * w0 and w1 are lane w of the first and of the second vector of the sweep's two-vector record (sweep_records.h): for an interior
 * node the address of the node its skip entry names - address of the first node + PTMI_SWEEP_NF_NODE_BYTES * index - and the
 * index of its right child (>= 0); for a leaf its first slot and -count.  Every float keeps its bits.  The primitive records stay
 * ptmi_sweep_prepare's.
 */
#ifndef PTMI_SWEEP_NEAR_FAR_H
#define PTMI_SWEEP_NEAR_FAR_H

#include "frame_block.h"

#define PTMI_SWEEP_NF_NODE_VECS 4
#define PTMI_SWEEP_NF_NODE_BYTES (PTMI_SWEEP_NF_NODE_VECS * PTMI_SWEEP_VEC_BYTES)
#define PTMI_SWEEP_NF_FAR_FIRST 8                     /* byte offset inside an axis group at which (hi, lo) stands */

/* The LDS image of a kernel that walks these records: [near/far nodes | primitives | frame block | materials] */
PTMI_HD size_t ptmi_sweep_near_far_lds_vecs(int n_nodes, int prim_stride, int n_prims) {
    return ptmi_sweep_lds_vecs(n_nodes, prim_stride, n_prims) + (PTMI_SWEEP_NF_NODE_VECS - 2) * (size_t)n_nodes;
}

/* The near/far node records, prepared from the scene's: records first, first + step, ... (a workgroup calls it with its thread
 * index and size, the host with 0 and 1).  nodes_at: the address the first of them will stand at.  in and out must not overlap. */
PTMI_HD void ptmi_sweep_near_far_prepare(const ptmi_vec_bits* nodes, int n_nodes, ptmi_vec_bits* out_nodes, uint32_t nodes_at, int first, int step) {
    int i;
    for (i = first; i < n_nodes; i += step) {
        const ptmi_vec_bits lo = nodes[2 * i], hi = nodes[2 * i + 1];
        ptmi_vec_bits* o = out_nodes + (size_t)PTMI_SWEEP_NF_NODE_VECS * i;
        const ptmi_vec_bits x = {lo.x, hi.x, hi.x, lo.x}, y = {lo.y, hi.y, hi.y, lo.y}, z = {lo.z, hi.z, hi.z, lo.z};
        ptmi_vec_bits w = {lo.w, hi.w, 0, 0};
        if ((int32_t)hi.w >= 0) w.x = nodes_at + lo.w * (uint32_t)PTMI_SWEEP_NF_NODE_BYTES;      /* interior: skip index -> address */
        o[0] = x; o[1] = y; o[2] = z; o[3] = w;
    }
}

#endif /* PTMI_SWEEP_NEAR_FAR_H */

/* sweep_records.h — the node and primitive records as the sweep walk (traversal.h: intersect_sweep) reads them from LDS, free of
 * HIP so that a plain C compiler can check the preparation on the host (tests/test_sweep_records_host.py) before a kernel walks it.
 *
 * The records in global memory, and what LANE and STACK stage, stay as SceneState::upload writes them.  The sweep's LDS copy
 * differs in two 32-bit lanes, so that its node and triangle passes do no bookkeeping of their own:
 *   an interior node's skip entry (lane w of its first vector) is the BYTE OFFSET of the node it names from the first node record,
 *       skip index * PTMI_SWEEP_NODE_BYTES: the sweep's cursor is such an offset and is itself the address of its LDS read, so
 *       the miss path is one select from the loaded lane.  The last skip entries name the node one past the end: the offset at
 *       which the walk is over;
 *   a primitive's slot lane (lane w of its second vector, zero in global memory and read by no walk) holds its leaf-order slot, so
 *       the hit update selects it from the register the record was loaded into.
 * Leaf nodes (first slot, -count) and every other lane are copied as they are.
 */
#ifndef PTMI_SWEEP_RECORDS_H
#define PTMI_SWEEP_RECORDS_H

#include <stddef.h>

#include "../../include/ptmi_math.h"

#define PTMI_SWEEP_VEC_BYTES 16                       /* one float4 */
#define PTMI_SWEEP_NODE_BYTES (2 * PTMI_SWEEP_VEC_BYTES)

/* one 16-byte vector of a record, by its bits */
typedef struct __attribute__((aligned(16))) { uint32_t x, y, z, w; } ptmi_vec_bits;

/* The scene's LDS image in 16-byte vectors: [nodes | primitives | materials], the same for every walk that stages the scene.
 * The one place that counts it: the host sizes the dynamic LDS from it, the kernels lay it out by it. */
PTMI_HD size_t ptmi_scene_lds_vecs(int n_nodes, int prim_stride, int n_prims) {
    return 2 * (size_t)n_nodes + ((size_t)prim_stride + 3) * (size_t)n_prims;
}

/* The sweep's node and primitive records, prepared from the scene's: records first, first + step, ... of both tables (a workgroup
 * calls it with its thread index and size, the host with 0 and 1).  in and out must not overlap. */
PTMI_HD void ptmi_sweep_prepare(const ptmi_vec_bits* nodes, int n_nodes, const ptmi_vec_bits* prims, int prim_stride, int n_prims,
                                ptmi_vec_bits* out_nodes, ptmi_vec_bits* out_prims, uint32_t nodes_at, int first, int step) {
    int i, k, c;
    for (i = first; i < n_nodes; i += step) {
        ptmi_vec_bits n0 = nodes[2 * i];
        const ptmi_vec_bits n1 = nodes[2 * i + 1];
        if ((int32_t)n1.w >= 0) n0.w = nodes_at + n0.w * (uint32_t)PTMI_SWEEP_NODE_BYTES;     /* interior: skip index -> address */
        out_nodes[2 * i] = n0;
        out_nodes[2 * i + 1] = n1;
    }
    for (k = first; k < n_prims; k += step) {
        const ptmi_vec_bits* r = prims + (size_t)prim_stride * k;
        ptmi_vec_bits* o = out_prims + (size_t)prim_stride * k;
        ptmi_vec_bits e1 = r[1];
        e1.w = (uint32_t)k;                                                        /* the slot lane */
        o[0] = r[0];
        o[1] = e1;
        for (c = 2; c < prim_stride; c++) o[c] = r[c];
    }
}

#endif

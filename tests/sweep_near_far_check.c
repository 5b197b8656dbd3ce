/* sweep_near_far_check.c — csrc/sweep_near_far.h on the host (tests/test_sweep_near_far_host.py builds and runs it).
 *   sweep_near_far_check <file>
 * <file>: the scenes of sweep_records_check.c, each  int32 n_nodes, prim_stride, n_prims; uint32 nodes_at;  then the node records
 * (2 * n_nodes vectors of 4 words) and the primitive records (prim_stride * n_prims vectors) as SceneState::upload lays them out.
 * For each scene ptmi_sweep_near_far_prepare runs once as the host calls it (0, 1) and once as a workgroup of 256 threads does, and
 *   - both give the same bytes;
 *   - each axis group of a record is lo, hi, hi, lo of the scene's node, bit for bit;
 *   - w1 (word 1 of the fourth vector) is lane w of the node's second vector, copied;
 *   - w0 (word 0) of an interior node is nodes_at + 64 * (the index it named), and that index lies in (i, n_nodes];
 *   - w0 of a leaf is copied; the two pad words are 0;
 *   - nothing is written outside the table (guard vectors on both sides);
 *   - ptmi_sweep_near_far_lds_vecs is what the layout [near/far nodes | primitives | frame block | materials] adds up to.
 * Prints "ok <scenes> <nodes>" or the first difference; exit status 0 / 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cuda-pathtracer_amd/csrc/sweep_near_far.h"

#define GUARD 4
#define THREADS 256

static int fail(const char* what, int scene, int at) {
    printf("scene %d: %s at %d\n", scene, what, at);
    return 1;
}

static int same(const ptmi_vec_bits* a, const ptmi_vec_bits* b) { return memcmp(a, b, sizeof *a) == 0; }

int main(int argc, char** argv) {
    FILE* f;
    int32_t head[3];
    int scene = 0;
    long nodes_seen = 0;
    if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
        fprintf(stderr, "usage: sweep_near_far_check <file>\n");
        return 2;
    }
    if (PTMI_SWEEP_NF_NODE_BYTES != 64 || PTMI_SWEEP_NF_FAR_FIRST != 8) return fail("the record is not 64 bytes with (hi, lo) at 8", 0, 0);
    while (fread(head, sizeof head, 1, f) == 1) {
        const int n_nodes = head[0], stride = head[1], n_prims = head[2];
        const size_t nv = 2 * (size_t)n_nodes, pv = (size_t)stride * n_prims, ov = 4 * (size_t)n_nodes;
        uint32_t nodes_at;
        ptmi_vec_bits *nodes, *out_a, *out_b, guard;
        int i, t;
        if (n_nodes < 1 || n_prims < 1 || (stride != 3 && stride != 4) || fread(&nodes_at, 4, 1, f) != 1) return fail("bad header", scene, 0);
        if (ptmi_sweep_near_far_lds_vecs(n_nodes, stride, n_prims) != ov + pv + PTMI_FRAME_BLOCK_VECS + 3 * (size_t)n_prims)
            return fail("ptmi_sweep_near_far_lds_vecs", scene, 0);
        nodes = (ptmi_vec_bits*)aligned_alloc(16, (nv + pv) * sizeof *nodes);
        out_a = (ptmi_vec_bits*)aligned_alloc(16, (ov + 2 * GUARD) * sizeof *nodes);
        out_b = (ptmi_vec_bits*)aligned_alloc(16, (ov + 2 * GUARD) * sizeof *nodes);
        if (!nodes || !out_a || !out_b || fread(nodes, sizeof *nodes, nv + pv, f) != nv + pv) return fail("short file", scene, 0);
        memset(&guard, 0xA5, sizeof guard);
        for (i = 0; i < (int)ov + 2 * GUARD; i++) out_a[i] = out_b[i] = guard;
        /* layout of out_*: GUARD | near/far nodes | GUARD */
        ptmi_sweep_near_far_prepare(nodes, n_nodes, out_a + GUARD, nodes_at, 0, 1);
        for (t = 0; t < THREADS; t++) ptmi_sweep_near_far_prepare(nodes, n_nodes, out_b + GUARD, nodes_at, t, THREADS);
        if (memcmp(out_a, out_b, (ov + 2 * GUARD) * sizeof *nodes)) return fail("the strided call differs from the whole one", scene, 0);
        for (i = 0; i < GUARD; i++)
            if (!same(&out_a[i], &guard) || !same(&out_a[GUARD + ov + i], &guard)) return fail("write outside the table", scene, i);
        for (i = 0; i < n_nodes; i++) {
            const ptmi_vec_bits lo = nodes[2 * i], hi = nodes[2 * i + 1], *o = out_a + GUARD + 4 * (size_t)i;
            const ptmi_vec_bits x = {lo.x, hi.x, hi.x, lo.x}, y = {lo.y, hi.y, hi.y, lo.y}, z = {lo.z, hi.z, hi.z, lo.z};
            if (!same(&o[0], &x) || !same(&o[1], &y) || !same(&o[2], &z)) return fail("an axis group is not lo, hi, hi, lo", scene, i);
            if (o[3].y != hi.w) return fail("w1 changed", scene, i);
            if (o[3].z != 0 || o[3].w != 0) return fail("a pad word is not 0", scene, i);
            if ((int32_t)hi.w >= 0) {                                                 /* interior */
                const uint32_t named = lo.w;
                if (named <= (uint32_t)i || named > (uint32_t)n_nodes) return fail("skip index out of (i, n_nodes]", scene, i);
                if (o[3].x != nodes_at + 64u * named) return fail("w0 of an interior node", scene, i);
            } else if (o[3].x != lo.w) {
                return fail("w0 of a leaf changed", scene, i);
            }
        }
        nodes_seen += n_nodes;
        free(nodes); free(out_a); free(out_b);
        scene++;
    }
    fclose(f);
    printf("ok %d %ld\n", scene, nodes_seen);
    return 0;
}

/* sweep_records_check.c — csrc/sweep_records.h on the host (tests/test_sweep_records_host.py builds and runs it).
 *   sweep_records_check <file>
 * <file>: any number of scenes, each  int32 n_nodes, prim_stride, n_prims; uint32 nodes_at;  then the node records
 * (2 * n_nodes vectors of 4 words) and the primitive records (prim_stride * n_prims vectors) as SceneState::upload lays them out.
 * For each scene ptmi_sweep_prepare runs once as the host calls it (0, 1) and once as a workgroup of 256 threads does, and
 *   - both give the same records;
 *   - an interior node's skip lane is nodes_at + 32 * (the index it named), and that index lies in (i, n_nodes];
 *   - a leaf node, and every other lane of an interior node, is copied as it is;
 *   - a primitive's slot lane (word 3 of its second vector) is its leaf-order slot, every other word is copied as it is;
 *   - nothing is written outside the two tables (guard vectors on both sides).
 * Prints "ok <scenes> <nodes> <prims>" or the first difference; exit status 0 / 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cuda-pathtracer_amd/csrc/sweep_records.h"

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
    long nodes_seen = 0, prims_seen = 0;
    if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
        fprintf(stderr, "usage: sweep_records_check <file>\n");
        return 2;
    }
    while (fread(head, sizeof head, 1, f) == 1) {
        const int n_nodes = head[0], stride = head[1], n_prims = head[2];
        const size_t nv = 2 * (size_t)n_nodes, pv = (size_t)stride * n_prims;
        uint32_t nodes_at;
        ptmi_vec_bits *nodes, *prims, *out_a, *out_b, guard;
        int i, k, c, t;
        if (n_nodes < 1 || n_prims < 1 || (stride != 3 && stride != 4) || fread(&nodes_at, 4, 1, f) != 1) return fail("bad header", scene, 0);
        if (ptmi_scene_lds_vecs(n_nodes, stride, n_prims) != nv + pv + 3 * (size_t)n_prims) return fail("ptmi_scene_lds_vecs", scene, 0);
        nodes = (ptmi_vec_bits*)aligned_alloc(16, (nv + pv) * sizeof *nodes);
        out_a = (ptmi_vec_bits*)aligned_alloc(16, (nv + pv + 3 * GUARD) * sizeof *nodes);
        out_b = (ptmi_vec_bits*)aligned_alloc(16, (nv + pv + 3 * GUARD) * sizeof *nodes);
        if (!nodes || !out_a || !out_b || fread(nodes, sizeof *nodes, nv + pv, f) != nv + pv) return fail("short file", scene, 0);
        prims = nodes + nv;
        memset(&guard, 0xA5, sizeof guard);
        for (i = 0; i < (int)(nv + pv) + 3 * GUARD; i++) out_a[i] = out_b[i] = guard;
        /* layout of out_*: GUARD | nodes | GUARD | prims | GUARD */
        ptmi_sweep_prepare(nodes, n_nodes, prims, stride, n_prims, out_a + GUARD, out_a + GUARD + nv + GUARD, nodes_at, 0, 1);
        for (t = 0; t < THREADS; t++)
            ptmi_sweep_prepare(nodes, n_nodes, prims, stride, n_prims, out_b + GUARD, out_b + GUARD + nv + GUARD, nodes_at, t, THREADS);
        if (memcmp(out_a, out_b, (nv + pv + 3 * GUARD) * sizeof *nodes)) return fail("the strided call differs from the whole one", scene, 0);
        for (i = 0; i < GUARD; i++)
            if (!same(&out_a[i], &guard) || !same(&out_a[GUARD + nv + i], &guard) || !same(&out_a[2 * GUARD + nv + pv + i], &guard))
                return fail("write outside the tables", scene, i);
        {
            const ptmi_vec_bits *on = out_a + GUARD, *op = out_a + 2 * GUARD + nv;
            for (i = 0; i < n_nodes; i++) {
                ptmi_vec_bits want = nodes[2 * i];
                if (!same(&on[2 * i + 1], &nodes[2 * i + 1])) return fail("second node vector changed", scene, i);
                if ((int32_t)nodes[2 * i + 1].w >= 0) {                                   /* interior */
                    const uint32_t named = nodes[2 * i].w;
                    if (named <= (uint32_t)i || named > (uint32_t)n_nodes) return fail("skip index out of (i, n_nodes]", scene, i);
                    want.w = nodes_at + 32u * named;
                }
                if (!same(&on[2 * i], &want)) return fail("first node vector", scene, i);
            }
            for (k = 0; k < n_prims; k++)
                for (c = 0; c < stride; c++) {
                    ptmi_vec_bits want = prims[(size_t)stride * k + c];
                    if (c == 1) {
                        if (want.w != 0) return fail("the slot lane is not free in the scene's record", scene, k);
                        want.w = (uint32_t)k;
                    }
                    if (!same(&op[(size_t)stride * k + c], &want)) return fail("primitive record", scene, k);
                }
        }
        nodes_seen += n_nodes; prims_seen += n_prims;
        free(nodes); free(out_a); free(out_b);
        scene++;
    }
    fclose(f);
    printf("ok %d %ld %ld\n", scene, nodes_seen, prims_seen);
    return 0;
}

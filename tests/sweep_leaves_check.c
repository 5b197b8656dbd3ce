/* sweep_leaves_check.c — csrc/sweep_leaves.h on the host (tests/test_sweep_leaves_host.py builds and runs it).
 *   sweep_leaves_check <file>
 * <file>: the scenes of sweep_records_check.c, each  int32 n_nodes, prim_stride, n_prims; uint32 at;  then the node records
 * (2 * n_nodes vectors of 4 words) and the primitive records (prim_stride * n_prims vectors) as SceneState::upload lays them out.
 * `at` is taken as the LDS address of the first primitive record.  For each scene ptmi_sweep_leaves_prepare runs once as the host
 * calls it (0, 1) and once as a workgroup of 256 threads does, and
 *   - both give the same bytes, and nothing is written outside the table (guard vectors on both sides);
 *   - record j is the j-th leaf of the node array in pre-order: its axis groups are lo, hi, hi, lo of that node, bit for bit;
 *   - the link vector is (rec, count, rec, count), rec = at + 16 * prim_stride * (the leaf's first slot), count = the leaf's;
 *   - the leaves' slots tile 0 .. n_prims in order (so the walk meets the primitives in the reference's order);
 *   - ptmi_sweep_leaf_count is the number of leaves and ptmi_sweep_leaves_lds_vecs is what
 *     [near/far nodes | primitives | frame block | materials | leaves] adds up to;
 *   - ptmi_sweep_leaves_verdict is 1 for the tree as built;
 *   - it is 0 after each of these changes to a copy, one at a time: for each of the six planes, a child's plane moved one ulp
 *     outside its parent's (on the first interior node; the left child for lo planes, the right child for hi planes and the other
 *     way round on every second scene, so both children are covered) - and 1 again with that plane exactly on its parent's; a
 *     plane of the last node set to +inf, -inf and NaN; a plane of the root set to NaN.  Trees of a single node have no child:
 *     only the non-finite changes apply.  And 0 for links whose ranges are consistent but which are not pre-order's: the root's right
 *     child moved one record further, the root's skip entry one short of the end (where the tree has room for either).
 * Prints "ok <scenes> <nodes> <leaves> <mutants>" or the first difference; exit status 0 / 1.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cuda-pathtracer_amd/csrc/sweep_leaves.h"

#define GUARD 4
#define THREADS 256

static int fail(const char* what, int scene, int at) {
    printf("scene %d: %s at %d\n", scene, what, at);
    return 1;
}

static int same(const ptmi_vec_bits* a, const ptmi_vec_bits* b) { return memcmp(a, b, sizeof *a) == 0; }

static uint32_t* plane_of(ptmi_vec_bits* nodes, int node, int plane) {      /* 0..2 lo.xyz, 3..5 hi.xyz */
    ptmi_vec_bits* v = nodes + 2 * node + plane / 3;
    return plane % 3 == 0 ? &v->x : plane % 3 == 1 ? &v->y : &v->z;
}

int main(int argc, char** argv) {
    FILE* f;
    int32_t head[3];
    int scene = 0;
    long nodes_seen = 0, leaves_seen = 0, mutants = 0;
    if (argc != 2 || !(f = fopen(argv[1], "rb"))) {
        fprintf(stderr, "usage: sweep_leaves_check <file>\n");
        return 2;
    }
    if (PTMI_SWEEP_LEAF_BYTES != 64 || PTMI_SWEEP_LEAF_LINK != 48) return fail("the record is not 64 bytes with the link at 48", 0, 0);
    while (fread(head, sizeof head, 1, f) == 1) {
        const int n_nodes = head[0], stride = head[1], n_prims = head[2];
        const size_t nv = 2 * (size_t)n_nodes, pv = (size_t)stride * n_prims;
        uint32_t at;
        ptmi_vec_bits *nodes, *copy, *out_a, *out_b, guard;
        int i, t, n_leaves, j = 0, slot = 0;
        size_t ov;
        if (n_nodes < 1 || n_prims < 1 || (stride != 3 && stride != 4) || fread(&at, 4, 1, f) != 1) return fail("bad header", scene, 0);
        nodes = (ptmi_vec_bits*)aligned_alloc(16, (nv + pv) * sizeof *nodes);
        copy = (ptmi_vec_bits*)aligned_alloc(16, nv * sizeof *nodes);
        if (!nodes || !copy || fread(nodes, sizeof *nodes, nv + pv, f) != nv + pv) return fail("short file", scene, 0);
        n_leaves = ptmi_sweep_leaf_count(nodes, n_nodes);
        for (i = 0, t = 0; i < n_nodes; i++) t += (int32_t)nodes[2 * i + 1].w < 0;
        if (n_leaves != t || n_leaves < 1) return fail("ptmi_sweep_leaf_count", scene, n_leaves);
        ov = 4 * (size_t)n_leaves;
        if (ptmi_sweep_leaves_lds_vecs(n_nodes, stride, n_prims, n_leaves) !=
            4 * (size_t)n_nodes + pv + PTMI_FRAME_BLOCK_VECS + 3 * (size_t)n_prims + ov) return fail("ptmi_sweep_leaves_lds_vecs", scene, 0);
        out_a = (ptmi_vec_bits*)aligned_alloc(16, (ov + 2 * GUARD) * sizeof *nodes);
        out_b = (ptmi_vec_bits*)aligned_alloc(16, (ov + 2 * GUARD) * sizeof *nodes);
        if (!out_a || !out_b) return fail("no memory", scene, 0);
        memset(&guard, 0xA5, sizeof guard);
        for (i = 0; i < (int)ov + 2 * GUARD; i++) out_a[i] = out_b[i] = guard;
        ptmi_sweep_leaves_prepare(nodes, n_nodes, stride, out_a + GUARD, at, 0, 1);
        for (t = 0; t < THREADS; t++) ptmi_sweep_leaves_prepare(nodes, n_nodes, stride, out_b + GUARD, at, t, THREADS);
        if (memcmp(out_a, out_b, (ov + 2 * GUARD) * sizeof *nodes)) return fail("the strided call differs from the whole one", scene, 0);
        for (i = 0; i < GUARD; i++)
            if (!same(&out_a[i], &guard) || !same(&out_a[GUARD + ov + i], &guard)) return fail("write outside the table", scene, i);
        for (i = 0; i < n_nodes; i++) {
            const ptmi_vec_bits lo = nodes[2 * i], hi = nodes[2 * i + 1], *o = out_a + GUARD + 4 * (size_t)j;
            const ptmi_vec_bits x = {lo.x, hi.x, hi.x, lo.x}, y = {lo.y, hi.y, hi.y, lo.y}, z = {lo.z, hi.z, hi.z, lo.z};
            uint32_t rec, count;
            if ((int32_t)hi.w >= 0) continue;
            if (j >= n_leaves) return fail("more leaves than counted", scene, i);
            if (!same(&o[0], &x) || !same(&o[1], &y) || !same(&o[2], &z)) return fail("an axis group is not lo, hi, hi, lo of the leaf in pre-order", scene, i);
            rec = at + 16u * (uint32_t)stride * lo.w; count = (uint32_t)(-(int32_t)hi.w);
            if (o[3].x != rec || o[3].z != rec) return fail("the first record's address", scene, i);
            if (o[3].y != count || o[3].w != count) return fail("the count", scene, i);
            if ((int)lo.w != slot) return fail("the leaves' slots do not tile the primitives in order", scene, i);
            slot += (int)count;
            j++;
        }
        if (j != n_leaves || slot != n_prims) return fail("leaves or slots left over", scene, j);
        if (ptmi_sweep_leaves_verdict(nodes, n_nodes, n_prims) != 1) return fail("the verdict of a built tree is not 1", scene, 0);
        /* constructed arrays: one change each */
        if (n_nodes > 1) {
            int interior = -1, plane;
            for (i = 0; i < n_nodes && interior < 0; i++)
                if ((int32_t)nodes[2 * i + 1].w >= 0) interior = i;
            if (interior != 0) return fail("the root of a tree of several nodes is a leaf", scene, interior);
            for (plane = 0; plane < 6; plane++) {
                const int use_right = (plane >= 3) ^ (scene & 1);
                const int child = use_right ? (int)nodes[2 * interior + 1].w : interior + 1;
                float parent, outside;
                memcpy(copy, nodes, nv * sizeof *nodes);
                memcpy(&parent, plane_of(copy, interior, plane), 4);
                outside = nextafterf(parent, plane < 3 ? -INFINITY : INFINITY);                 /* one ulp outside the parent's */
                memcpy(plane_of(copy, child, plane), &outside, 4);
                if (ptmi_sweep_leaves_verdict(copy, n_nodes, n_prims) != 0) return fail("a child plane one ulp outside passes", scene, plane);
                memcpy(plane_of(copy, child, plane), &parent, 4);            /* on the parent's plane: contained, and it still holds its own children */
                if (ptmi_sweep_leaves_verdict(copy, n_nodes, n_prims) != 1) return fail("a child plane on its parent's fails", scene, plane);
                mutants++;
            }
        }
        {
            const uint32_t bad[3] = {0x7f800000u, 0xff800000u, 0x7fc00000u};
            int b, plane;
            for (b = 0; b < 3; b++)
                for (plane = 0; plane < 6; plane++) {
                    memcpy(copy, nodes, nv * sizeof *nodes);
                    *plane_of(copy, n_nodes - 1, plane) = bad[b];
                    if (ptmi_sweep_leaves_verdict(copy, n_nodes, n_prims) != 0) return fail("a non-finite plane of the last node passes", scene, 6 * b + plane);
                    mutants++;
                }
            for (plane = 0; plane < 6; plane++) {
                memcpy(copy, nodes, nv * sizeof *nodes);
                *plane_of(copy, 0, plane) = bad[2];
                if (ptmi_sweep_leaves_verdict(copy, n_nodes, n_prims) != 0) return fail("a NaN plane of the root passes", scene, plane);
                mutants++;
            }
        }
        /* links with consistent ranges that are not pre-order's: the root's right child one further, its skip entry one short */
        if (n_nodes > 1) {
            const uint32_t right = nodes[1].w, skip = nodes[0].w;
            if (right + 1 < skip) {
                memcpy(copy, nodes, nv * sizeof *nodes);
                copy[1].w = right + 1;
                if (ptmi_sweep_leaves_verdict(copy, n_nodes, n_prims) != 0) return fail("a right child behind the left subtree's end passes", scene, 0);
                mutants++;
            }
            if (skip - 1 > right) {
                memcpy(copy, nodes, nv * sizeof *nodes);
                copy[0].w = skip - 1;
                if (ptmi_sweep_leaves_verdict(copy, n_nodes, n_prims) != 0) return fail("a skip entry short of the subtree's end passes", scene, 0);
                mutants++;
            }
        }
        nodes_seen += n_nodes; leaves_seen += n_leaves;
        free(nodes); free(copy); free(out_a); free(out_b);
        scene++;
    }
    fclose(f);
    printf("ok %d %ld %ld %ld\n", scene, nodes_seen, leaves_seen, mutants);
    return 0;
}

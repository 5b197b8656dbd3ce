/* frame_block_check.c — csrc/frame_block.h on the host (tests/test_frame_block_host.py builds and runs it).
 *   frame_block_check <in> <out>
 * <in>: any number of cases, each 12 floats (the camera's org, llc, hor, ver) and 2 int32 (width, height).
 * For each case the block is packed as the kernels pack it - ptmi_frame_block_pack with the reciprocals of ptmi_size_reciprocal
 * (shade_lean.h), which is what the host puts into TileMap - between guard vectors, and written to <out>: 4 vectors of 4 words.
 * The test compares them with the layout it lays out itself.  Here: nothing is written outside the block, a second call gives the
 * same block, and ptmi_sweep_lds_vecs counts it.  Prints "ok <cases>" or the first complaint; exit status 0 / 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cuda-pathtracer_amd/csrc/frame_block.h"
#include "../cuda-pathtracer_amd/csrc/shade_lean.h"

#define GUARD 2

int main(int argc, char** argv) {
    FILE *in, *out;
    float cam[12];
    int32_t size[2];
    int cases = 0, i;
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) {
        fprintf(stderr, "usage: frame_block_check <in> <out>\n");
        return 2;
    }
    if (ptmi_sweep_lds_vecs(5, 3, 7) != ptmi_scene_lds_vecs(5, 3, 7) + PTMI_FRAME_BLOCK_VECS || PTMI_FRAME_BLOCK_VECS * sizeof(ptmi_vec_bits) >= 128) {
        printf("ptmi_sweep_lds_vecs does not count the block, or the block is not under 128 bytes\n");
        return 1;
    }
    while (fread(cam, sizeof cam, 1, in) == 1 && fread(size, sizeof size, 1, in) == 1) {
        ptmi_vec_bits a[PTMI_FRAME_BLOCK_VECS + 2 * GUARD], b[PTMI_FRAME_BLOCK_VECS + 2 * GUARD], guard;
        const float inv_w = ptmi_size_reciprocal(size[0]), inv_h = ptmi_size_reciprocal(size[1]);
        memset(&guard, 0xA5, sizeof guard);
        for (i = 0; i < PTMI_FRAME_BLOCK_VECS + 2 * GUARD; i++) a[i] = b[i] = guard;
        ptmi_frame_block_pack(cam, cam + 3, cam + 6, cam + 9, size[0], size[1], inv_w, inv_h, a + GUARD);
        ptmi_frame_block_pack(cam, cam + 3, cam + 6, cam + 9, size[0], size[1], inv_w, inv_h, b + GUARD);
        if (memcmp(a, b, sizeof a)) { printf("case %d: two calls differ\n", cases); return 1; }
        for (i = 0; i < GUARD; i++)
            if (memcmp(&a[i], &guard, sizeof guard) || memcmp(&a[GUARD + PTMI_FRAME_BLOCK_VECS + i], &guard, sizeof guard)) {
                printf("case %d: write outside the block\n", cases);
                return 1;
            }
        if (fwrite(a + GUARD, sizeof guard, PTMI_FRAME_BLOCK_VECS, out) != PTMI_FRAME_BLOCK_VECS) return 2;
        cases++;
    }
    fclose(in);
    if (fclose(out)) return 2;
    printf("ok %d\n", cases);
    return 0;
}

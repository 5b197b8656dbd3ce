/* frame_block.h — the frame's constants as the sweep's shade step reads them from LDS (shading.h: camera_dir_block), free of HIP
 * so that a plain C compiler can check the packer on the host (tests/test_frame_block_host.py).
 *
 * The camera and the image size are the same for every segment of a launch, and the next camera ray is the one place of the
 * segment loop that reads them.  As kernel arguments they take 18 scalar registers the loop does not have: the compiler parks
 * some in the lanes of a vector register and fetches others again from the argument block in every segment.  The sweep's kernels
 * therefore stage them once per workgroup, with the scene (bounce.h: stage_scene), and the camera branch reads four broadcast
 * vectors.  Each field keeps its bits: the block is a copy, nothing is computed from it in advance but the two int -> float
 * conversions of the image size, which are exact or correctly rounded either way.
 *
 *   vector 0   llc.x   llc.y   llc.z   (float)width
 *   vector 1   hor.x   hor.y   hor.z   inv_width       (TileMap: ptmi_size_reciprocal(width), or 0)
 *   vector 2   ver.x   ver.y   ver.z   (float)height
 *   vector 3   org.x   org.y   org.z   inv_height
 */
#ifndef PTMI_FRAME_BLOCK_H
#define PTMI_FRAME_BLOCK_H

#include "sweep_records.h"

#define PTMI_FRAME_BLOCK_VECS 4

/* The LDS image of a kernel that walks with the sweep: [nodes | primitives | frame block | materials].  The block stands in front
 * of the materials so that one base address serves both (a material vector is the block's address + a constant + 48 * slot). */
PTMI_HD size_t ptmi_sweep_lds_vecs(int n_nodes, int prim_stride, int n_prims) {
    return ptmi_scene_lds_vecs(n_nodes, prim_stride, n_prims) + PTMI_FRAME_BLOCK_VECS;
}

PTMI_HD uint32_t ptmi_f2u(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }

/* The block of one frame.  The kernel, the intersect hook's staging and the host check all call this one function. */
PTMI_HD void ptmi_frame_block_pack(const float org[3], const float llc[3], const float hor[3], const float ver[3], int width, int height,
                                   float inv_width, float inv_height, ptmi_vec_bits out[PTMI_FRAME_BLOCK_VECS]) {
    const ptmi_vec_bits v0 = {ptmi_f2u(llc[0]), ptmi_f2u(llc[1]), ptmi_f2u(llc[2]), ptmi_f2u((float)width)};
    const ptmi_vec_bits v1 = {ptmi_f2u(hor[0]), ptmi_f2u(hor[1]), ptmi_f2u(hor[2]), ptmi_f2u(inv_width)};
    const ptmi_vec_bits v2 = {ptmi_f2u(ver[0]), ptmi_f2u(ver[1]), ptmi_f2u(ver[2]), ptmi_f2u((float)height)};
    const ptmi_vec_bits v3 = {ptmi_f2u(org[0]), ptmi_f2u(org[1]), ptmi_f2u(org[2]), ptmi_f2u(inv_height)};
    out[0] = v0; out[1] = v1; out[2] = v2; out[3] = v3;
}

#endif /* PTMI_FRAME_BLOCK_H */

// lens.h — the primary ray of a thin lens (include/ptmi.h: "thin lens"; the block: host/lens.cpp), as ptmi_render_nee forms it
// per sample and as the test hook (debug_hooks.hip: ptmi_debug_lens_ray_k) forms it once per case.  binary32, uncontracted
// (-ffp-contract=off), in the order the header writes.  The ray is the sensor's get_ray over the per-sample frame
// (o, llc_f, hor_f, ver_f): camera_ray's expressions on other operands.
#pragma once
#include "shading.h"

namespace ptmi {

// The six records are read here, where they are used, and not by the caller in front of its sample loop: the block's address is
// wave-uniform, so these are scalar loads into registers that are free again at the end of the function, and nothing of the
// lens lives across a walk.
//   r3, r4: the lens draws.  rho = sqrt(r3) and phi = (float)(2 pi r4) in the forms cosine_hemisphere has them: r3 is a curand
//     uniform, in [2^-33, 1], where sqrt_lean gives sqrt_rn's bits.
//   r1, r2: the jitter draws; u and v by the IEEE divisions camera_dir_raw makes in this kernel.
__device__ __forceinline__ void lens_ray_at(const float4* __restrict__ lens, int x, int y, float r3, float r4, float r1, float r2, f3& o, f3& d) {
    const float4 b0 = lens[0], b1 = lens[1], b2 = lens[2], b3 = lens[3], b4 = lens[4], b5 = lens[5];   // (llc_f, W) (hor_f, 1/W) (ver_f, H) (org, 1/H) (a, 0) (b, 0)
    const float rho = sqrt_lean(r3);
    const float phi = (float)((double)2.0f * PTMI_PI_D * (double)r4);
    float sphi, cphi;
    ptmi_sincosf(phi, &sphi, &cphi);
    const float dx = rho * cphi;
    const float dy = rho * sphi;
    o = xyz(b3) + dx * xyz(b4) + dy * xyz(b5);
    const float u = ((float)x + r1) / b0.w;
    const float v = ((float)y + r2) / b2.w;
    d = unit_vector(xyz(b0) + u * xyz(b1) + v * xyz(b2) - o);
}

// the four draws of a lens sample, the lens's first, and the ray
__device__ __forceinline__ void lens_ray(const float4* __restrict__ lens, int x, int y, Rng& rng, f3& o, f3& d) {
    const float r3 = rng_uniform(rng);
    const float r4 = rng_uniform(rng);
    const float r1 = rng_uniform(rng);
    const float r2 = rng_uniform(rng);
    lens_ray_at(lens, x, y, r3, r4, r1, r2, o, d);
}

}  // namespace ptmi

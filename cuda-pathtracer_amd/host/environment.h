// environment.h — host half of the environment light (include/ptmi.h: "environment lighting"): the parameter check and the
// sampling table of a lat-long radiance map.  No device involved; ptmi_host_env_table exposes the builder.
#pragma once
#include <vector>

namespace ptmi {

struct EnvParams {
    float scale = 1.0f;            // every texel is multiplied by it on upload
    float rotation_deg = 0.0f;     // the map turned about +y
    float select_fraction = 0.5f;  // with next_event: probability that a vertex's light sample goes to the environment
};

// The table of one map, exactly as include/ptmi.h writes it: z (h + 1), float CDFs built from binary64 running sums, and
// per texel the scaled radiance with the pdf per solid angle DERIVED FROM THE STORED CDFs.
struct EnvHostTable {
    int width = 0, height = 0;
    std::vector<float> z;          // h + 1: z_0 = 1 ... z_h = -1
    std::vector<float> marginal;   // h
    std::vector<float> row_cdf;    // h * w
    std::vector<float> texel;      // h * w * 4: (E.xyz, pdf)
    float total = 0.0f;
    float rot_turns = 0.0f;        // rotation_deg / 360.0f
};

void checkEnvParams(const EnvParams& p);                                       // throws ArgError
// throws ArgError for a bad size, a negative / NaN / infinite texel (before or after the scale) or a total that is not finite
void buildEnvTable(int width, int height, const float* rgb, const EnvParams& p, EnvHostTable& out);

}  // namespace ptmi

// environment.cpp — the sampling table of a lat-long radiance map, in the order include/ptmi.h ("environment lighting") writes it.
#include "environment.h"

#include <cmath>
#include <string>

#include "application_state.h"   // ArgError; brings in the HIP runtime that ptmi_math.h's qualifiers need
#include "../../include/ptmi_math.h"

namespace ptmi {

void checkEnvParams(const EnvParams& p) {
    if (!(p.scale >= 0.0f && std::isfinite(p.scale))) throw ArgError("environment: scale must be finite and >= 0");
    if (!(p.rotation_deg >= -360.0f && p.rotation_deg <= 360.0f)) throw ArgError("environment: rotation_deg must be in [-360, 360]");
    if (!(p.select_fraction >= 0.0f && p.select_fraction <= 1.0f)) throw ArgError("environment: select_fraction must be in [0, 1]");
}

void buildEnvTable(int w, int h, const float* rgb, const EnvParams& p, EnvHostTable& t) {
    checkEnvParams(p);
    if (w < 1 || h < 1) throw ArgError("environment: width and height must be >= 1");
    if ((long long)w * (long long)h > (1ll << 25)) throw ArgError("environment: width * height must be <= 2^25");
    if (!rgb) throw ArgError("environment: rgb is NULL");
    const size_t n = (size_t)w * (size_t)h;
    t.width = w; t.height = h;
    t.rot_turns = p.rotation_deg / 360.0f;
    t.z.assign((size_t)h + 1, 0.0f);
    for (int r = 0; r <= h; r++) {
        double s, c;
        ptmi_sincos_d((PTMI_PI_D * (double)r) / (double)h, &s, &c);
        t.z[r] = (float)c;
    }
    t.z[0] = 1.0f; t.z[h] = -1.0f;
    t.texel.assign(n * 4, 0.0f);
    for (size_t i = 0; i < n; i++) {
        for (int ch = 0; ch < 3; ch++) {
            const float raw = rgb[3 * i + ch];
            const float e = raw * p.scale;
            if (!(raw >= 0.0f && std::isfinite(raw) && std::isfinite(e)))
                throw ArgError("environment: texel " + std::to_string(i) + " is negative, NaN or infinite");
            t.texel[4 * i + ch] = e;
        }
    }
    // binary64 running sums: per row over the texel weights, then over the row totals
    std::vector<double> run(n), row_total((size_t)h), omega((size_t)h), mrun((size_t)h);
    double total = 0.0;
    for (int r = 0; r < h; r++) {
        omega[r] = ((2.0 * PTMI_PI_D) / (double)w) * ((double)t.z[r] - (double)t.z[r + 1]);
        double acc = 0.0;
        for (int j = 0; j < w; j++) {
            const float* e = &t.texel[4 * ((size_t)r * w + j)];
            acc = acc + omega[r] * (((double)e[0] + (double)e[1]) + (double)e[2]);
            run[(size_t)r * w + j] = acc;
        }
        row_total[r] = acc;
        total = total + acc;
        mrun[r] = total;
    }
    t.total = (float)total;
    if (!std::isfinite(t.total)) throw ArgError("environment: the map's total power overflows float");
    // float CDFs that end at exactly 1; an empty row (or map) keeps an all-zero CDF and is never selected
    t.marginal.assign((size_t)h, 0.0f);
    t.row_cdf.assign(n, 0.0f);
    for (int r = 0; r < h; r++) {
        if (total > 0.0) t.marginal[r] = (float)(mrun[r] / total);
        if (row_total[r] > 0.0)
            for (int j = 0; j < w; j++) t.row_cdf[(size_t)r * w + j] = (float)(run[(size_t)r * w + j] / row_total[r]);
    }
    // the pdf of texel (r, j) is the probability with which the two searches over the STORED floats pick it, over its solid angle
    for (int r = 0; r < h; r++) {
        const double pm = (double)t.marginal[r] - (r > 0 ? (double)t.marginal[r - 1] : 0.0);
        for (int j = 0; j < w; j++) {
            const size_t i = (size_t)r * w + j;
            const double pc = (double)t.row_cdf[i] - (j > 0 ? (double)t.row_cdf[i - 1] : 0.0);
            const double prob = pm * pc;
            t.texel[4 * i + 3] = prob > 0.0 ? (float)(prob / omega[r]) : 0.0f;
        }
    }
}

}  // namespace ptmi

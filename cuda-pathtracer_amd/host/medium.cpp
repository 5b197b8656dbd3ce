// medium.cpp — the check of a participating medium's numbers and the medium block, as include/ptmi.h ("participating medium")
// states them.
#include "medium.h"

#include <cmath>
#include <string>

namespace ptmi {

namespace {
const char* const kAxis[3] = {"x", "y", "z"};
const char* const kChannel[3] = {"r", "g", "b"};
}  // namespace

void checkMedium(const Medium& m) {
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(m.lo[a])) throw MediumError(std::string("medium: lo.") + kAxis[a] + " is not finite");
        if (!std::isfinite(m.hi[a])) throw MediumError(std::string("medium: hi.") + kAxis[a] + " is not finite");
    }
    if (!std::isfinite(m.sigma_t)) throw MediumError("medium: sigma_t is not finite");
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(m.albedo[c])) throw MediumError(std::string("medium: albedo.") + kChannel[c] + " is not finite");
    if (!std::isfinite(m.g)) throw MediumError("medium: g is not finite");
    for (int a = 0; a < 3; a++)
        if (!(m.lo[a] < m.hi[a])) throw MediumError(std::string("medium: the box is empty: lo.") + kAxis[a] + " must be below hi." + kAxis[a]);
    if (m.sigma_t < 0.0f) throw MediumError("medium: sigma_t must not be negative");
    for (int c = 0; c < 3; c++)
        if (m.albedo[c] < 0.0f || m.albedo[c] > 1.0f) throw MediumError(std::string("medium: albedo.") + kChannel[c] + " must lie in [0, 1]");
    if (std::fabs(m.g) > 0.9f) throw MediumError("medium: |g| must not exceed 0.9");
}

void mediumBlock(const Medium& m, float out12[kMediumBlockFloats]) {
    if (!out12) throw MediumError("medium: NULL argument");
    checkMedium(m);
    for (int k = 0; k < 3; k++) {
        out12[k] = m.lo[k];
        out12[4 + k] = m.hi[k];
        out12[8 + k] = m.albedo[k];
    }
    out12[3] = m.sigma_t; out12[7] = m.g; out12[11] = 0.0f;
}

void mediumCorners(const Medium& m, float out24[24]) {
    for (int i = 0; i < 8; i++)
        for (int a = 0; a < 3; a++) out24[3 * i + a] = (i >> a) & 1 ? m.hi[a] : m.lo[a];
}

}  // namespace ptmi

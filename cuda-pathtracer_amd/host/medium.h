// medium.h — host half of the participating medium (include/ptmi.h: "participating medium"): the check of a caller's medium and
// the medium block the per-lane kernel reads.  No device and no HIP header involved, so the file can be built and tested alone
// (tests/medium_check.cpp); ptmi_check_medium and ptmi_host_medium_block expose both.
#pragma once
#include <stdexcept>

namespace ptmi {

constexpr int kMediumBlockFloats = 12;                        // three float4: (lo, sigma_t) (hi, g) (albedo, 0)

// the caller's numbers (ptmi_medium of include/ptmi.h, field for field)
struct Medium {
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {1.0f, 1.0f, 1.0f};
    float sigma_t = 0.0f;                                     // 0: no medium
    float albedo[3] = {1.0f, 1.0f, 1.0f};
    float g = 0.0f;
};

// what the functions below throw; the C ABI reports it as PTMI_E_INVALID with the message
struct MediumError : std::invalid_argument { using std::invalid_argument::invalid_argument; };

// throws MediumError: a field that is not finite, lo >= hi on an axis, a negative sigma_t, an albedo outside [0, 1], |g| > 0.9
void checkMedium(const Medium& m);

// the block of a medium (checked as above): the caller's numbers, unchanged
void mediumBlock(const Medium& m, float out12[kMediumBlockFloats]);

// the eight corners of the box, 24 floats: what a scene with quads holds to its bound on ray origins (SceneState::checkQuadOrigin)
void mediumCorners(const Medium& m, float out24[24]);

}  // namespace ptmi

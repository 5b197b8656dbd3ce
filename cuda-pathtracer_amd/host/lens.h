// lens.h — host half of the thin lens (include/ptmi.h: "thin lens"): the check of a caller's radius and focus distance and the
// lens block the per-lane kernel reads, derived from a camera frame.  No device and no HIP header involved, so the file can be
// built and tested alone (tests/lens_check.cpp); ptmi_check_lens and ptmi_host_lens_block expose both.
#pragma once
#include <stdexcept>

namespace ptmi {

constexpr int kLensBlockFloats = 24;                          // six float4: (llc_f, W) (hor_f, 1/W) (ver_f, H) (org, 1/H) (a, 0) (b, 0)

// what the functions below throw; the C ABI reports it as PTMI_E_INVALID with the message
struct LensError : std::invalid_argument { using std::invalid_argument::invalid_argument; };

// throws LensError: a radius or focus distance that is a NaN or infinite, a negative radius, a focus distance that is not positive
void checkLens(float radius, float focus_distance);

// The block of a lens (radius > 0, checked as above) over the frame (org, llc, hor, ver) of ptmi_get_camera_frame and an image of
// width x height pixels; binary32, every operation rounded, in the order include/ptmi.h writes.  Throws LensError where width or
// height is not positive or a value of the block is not finite (f * hor overflows, hor or ver has no length).
void lensBlock(const float frame12[12], int width, int height, float radius, float focus_distance, float out24[kLensBlockFloats]);

}  // namespace ptmi

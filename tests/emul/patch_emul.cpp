// patch_emul.cpp -- host build of the patch core (opencv-ar_amd/csrc/patch_core.h) for the patch tests: the sequential
// reference patch_extract_frame, which the kernel of patch.hip must match byte for byte.
#include "patch_core.h"

using namespace ocvar;

extern "C" {

// One frame's `slots` patch slots and statuses (status may be NULL) under its records.  Returns the number of slots written.
int patch_extract_frame_emul(const uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* recs, int count, int slots,
                             uint8_t* patches, int pw, int ph, int flags, int* status) {
    return patch_extract_frame(frame, W, H, row_stride, fmt, recs, count, slots, patches, pw, ph, flags, status);
}

// The float32 map of a square (9 floats); 0: it has none.
int patch_map32_emul(const float* square, int pw, int ph, float* m32) { return perspective_from_quad(square, pw, ph, m32) ? 1 : 0; }

}  // extern "C"

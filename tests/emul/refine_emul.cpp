// refine_emul.cpp -- host build of the corner refinement core (opencv-ar_amd/csrc/refine_core.h) for the corner refinement
// tests: the same equations, summation order and reduction tree as refine_corners_kernel, on a row-major grey image.
#include "refine_core.h"
#include <vector>

using namespace ocvar;

extern "C" {

// the weights g[0 .. 2w] of a setting, as the context computes them
void refine_weights(int half_win, float* g) {
    const RefineArgs a = refine_args_make(half_win, 1, 0.0f);
    for (int k = 0; k < 2 * half_win + 1; k++) g[k] = a.g[k];
}

// refine n corners xy[2n] in place on a W x H grey image (row stride `stride` bytes)
void refine_points(const uint8_t* gray, int W, int H, int stride, float* xy, int n, int half_win, int max_iter, float eps) {
    const RefineArgs ra = refine_args_make(half_win, max_iter, eps);
    std::vector<float> P((size_t)refine_patch_side(half_win) * refine_patch_side(half_win));
    auto px = [=](int x, int y) -> int { return gray[(size_t)y * stride + x]; };
    for (int k = 0; k < n; k++) refine_corner(px, W, H, ra, P.data(), xy[2 * k], xy[2 * k + 1]);
}

}  // extern "C"

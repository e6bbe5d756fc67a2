// refine.hip -- opt-in sub-pixel refinement of the output markers' corners (ocvar_hip_set_corner_refine), between
// finalise_kernel (the marker records and their pose job list) and pose_kernel (which then solves from the refined corners).
// The equations, the summation order and the reduction tree are refine_core.h's; the host build of that file reproduces
// this kernel bit for bit (tests/emul/refine_emul.cpp).
#include "kernels.h"

namespace ocvar {

// One wave per marker, walking the batch's pose jobs (their count is known only on the device) with a grid-stride loop; one
// 16-lane row per corner.  Each step a row samples its (2w+3)^2 patch into LDS (at most 33^2 floats: 4.3 KB a row), takes its
// partial sums over the interior points (refine_partial) and combines them with a butterfly of shuffles inside the row, which
// leaves refine_tree's value in all 16 lanes; every lane then takes the same step.  The wave loops until its four rows have
// stopped.  Tracked and new markers alike: the record's square is this frame's.
__global__ __launch_bounds__(64) void refine_corners_kernel(Workspace ws, RefineArgs ra) {
    extern __shared__ float s_patch[];   // [4][(2w+3)^2]
    const int w = ra.half_win;
    const int side = refine_patch_side(w);
    const int row = threadIdx.x >> 4, l = threadIdx.x & (REFINE_LANES - 1);
    float* P = s_patch + row * side * side;
    int n = ws.counters[CNT_POSE_JOBS];
    const int cap = ws.n_frames * ws.maxm;
    if (n > cap) n = cap;
    const int W = ws.W, H = ws.H, pitch = gray_pitch(ws.W);
    const long long plane_bytes = gray_plane_bytes(ws.W, ws.H);
    for (int j = blockIdx.x; j < n; j += gridDim.x) {   // (uniform across the wave)
        const int job = ws.pose_jobs[j];
        const int f = job / ws.maxm;
        MarkerRec* m = ws.markers + job;
        const uint8_t* plane = ws.gray + (size_t)f * plane_bytes;
        auto px = [=](int x, int y) -> int { return plane[(size_t)y * pitch + gray_col(x)]; };
        const float x0 = m->square[2 * row], y0 = m->square[2 * row + 1];
        float cx = x0, cy = y0;
        bool active = true;
        int iter = 0;
        while (__ballot(active) != 0ull) {
            if (active) refine_sample(px, W, H, w, cx, cy, P, l, REFINE_LANES);
            __syncthreads();
            double s[5];
            if (active) refine_partial(P, ra.g, w, l, s);
            else for (int q = 0; q < 5; q++) s[q] = 0.0;
            for (int mask = REFINE_LANES / 2; mask >= 1; mask >>= 1)
                for (int q = 0; q < 5; q++) s[q] = s[q] + __shfl_xor(s[q], mask, REFINE_LANES);
            if (active) {
                const bool stop = refine_update(s, cx, cy, W, H, ra.eps2);
                iter++;
                if (stop || iter >= ra.max_iter) active = false;
            }
            __syncthreads();   // (the next step overwrites the patch)
        }
        refine_finish(x0, y0, w, cx, cy);
        if (l == 0) {
            m->square[2 * row] = cx;
            m->square[2 * row + 1] = cy;
        }
    }
}

void launch_refine_corners(const Workspace& ws, const RefineArgs& refine, hipStream_t stream) {
    if (ws.n_frames <= 0 || refine.half_win <= 0) return;
    const int side = refine_patch_side(refine.half_win);
    const long long cap = (long long)ws.n_frames * ws.maxm;
    const int blocks = (int)(cap < 4096 ? cap : 4096);
    hipLaunchKernelGGL(refine_corners_kernel, dim3(blocks), dim3(64), (size_t)4 * side * side * sizeof(float), stream, ws, refine);
}

}  // namespace ocvar

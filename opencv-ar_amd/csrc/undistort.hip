// undistort.hip -- opt-in undistortion of device-resident frames and marker records with the context's lens model
// (ocvar_hip_undistort / ocvar_hip_undistort_records).  The definition is undistort_core.h's; its host build
// (tests/emul/undistort_emul.cpp) gives these kernels' bytes.  No workspace and no precomputed map: every lane computes the lens
// model of its pixels in FP64 (about 40 operations per pixel against the 8 bytes per pixel a map would add to the traffic).  The
// camera travels by value in the launch arguments, so a later ocvar_hip_set_camera cannot race a queued launch.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int UNDIST_LANE_PX = 4;                       // consecutive destination pixels of one row a lane owns: 4, 12 or 16 bytes
constexpr int UNDIST_WAVE_PX = 64 * UNDIST_LANE_PX;     // destination pixels of one wave's span

// A one-wave workgroup owns a span of UNDIST_WAVE_PX pixels of one destination row (blockIdx: span, row, frame); a lane owns
// UNDIST_LANE_PX consecutive ones, whose source position is computed once per pixel.  A lane's bytes are put together in
// registers.  ALIGNED (the destination's address, row stride and frame stride are multiples of 4): they are BPP whole dwords
// and stored as such, except in the lane that crosses the row's end; everything else goes byte by byte.
template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(64) void undistort_kernel(UndistortArgs a) {
    const int u0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * UNDIST_LANE_PX;
    const int v = blockIdx.y;
    if (u0 >= a.W) return;
    const uint8_t* src = a.src + (size_t)blockIdx.z * a.src_frame_stride;
    uint8_t* out = a.dst + (size_t)blockIdx.z * a.dst_frame_stride + (long long)v * a.dst_row_stride + (long long)u0 * BPP;
    unsigned q[BPP];
    OCVAR_UNROLL
    for (int j = 0; j < BPP; j++) q[j] = 0;
    OCVAR_UNROLL
    for (int i = 0; i < UNDIST_LANE_PX; i++) {
        if (u0 + i < a.W) {
            int X, Y;
            undistort_source_fixed(a.cam, u0 + i, v, &X, &Y);
            OCVAR_UNROLL
            for (int c = 0; c < BPP; c++) {
                run_put(q, i * BPP + c, undistort_sample(src, a.W, a.H, a.src_row_stride, BPP, c, X, Y) & 255);
            }
        }
    }
    if (ALIGNED && u0 + UNDIST_LANE_PX <= a.W) {
        run_store(q, out, true, 0);
    } else {   // (pixel by pixel: a lane's pixels end where the row does)
        OCVAR_UNROLL
        for (int i = 0; i < UNDIST_LANE_PX; i++)
            if (u0 + i < a.W) {
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) out[i * BPP + c] = (uint8_t)run_byte(q, i * BPP + c);
            }
    }
}

template <int BPP>
static void launch_bpp(const UndistortArgs& a, int n_frames, bool aligned, hipStream_t stream) {
    const dim3 grid((a.W + UNDIST_WAVE_PX - 1) / UNDIST_WAVE_PX, a.H, n_frames);
    if (aligned)
        hipLaunchKernelGGL((undistort_kernel<BPP, true>), grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((undistort_kernel<BPP, false>), grid, dim3(64), 0, stream, a);
}

void launch_undistort(const UndistortArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || a.W <= 0 || a.H <= 0) return;
    const int bpp = format_bpp(format);
    const bool aligned = frames_dwords(a.dst, a.dst_row_stride, a.dst_frame_stride);
    switch (bpp) {
        case 1: launch_bpp<1>(a, n_frames, aligned, stream); break;
        case 3: launch_bpp<3>(a, n_frames, aligned, stream); break;
        case 4: launch_bpp<4>(a, n_frames, aligned, stream); break;
        default: break;
    }
}

// One lane per record slot k < min(count, slots) of every frame (blockIdx: 64 slots, frame); the other slots are not written.
// A lane reads its record before it writes it, so out may be in.
__global__ __launch_bounds__(64) void undistort_records_kernel(UndistortRecArgs a) {
    const int k = (int)blockIdx.x * 64 + (int)threadIdx.x, f = blockIdx.y;
    int n = a.counts[f];
    n = n < a.slots ? n : a.slots;
    if (k >= n) return;
    MarkerRec r = a.in[(size_t)f * a.slots + k];
    undistort_square(a.cam, r.square, r.square);
    a.out[(size_t)f * a.slots + k] = r;
}

void launch_undistort_records(const UndistortRecArgs& a, int n_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.slots <= 0) return;
    hipLaunchKernelGGL(undistort_records_kernel, dim3((a.slots + 63) / 64, n_frames), dim3(64), 0, stream, a);
}

}  // namespace ocvar

// patch.hip -- opt-in extraction of the rectified image of every marker of device-resident frames (ocvar_hip_patches /
// ocvar_hip_patches_records).  The definition is patch_core.h's; its host build (tests/emul/patch_emul.cpp) gives this
// kernel's bytes.  One launch per chunk of frames, no workspace: every wave recomputes its record's map.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int PATCH_LANE_PX = 4;                      // consecutive stored pixels a lane owns: 4, 12 or 16 bytes, whole dwords
constexpr int PATCH_WAVE_PX = 64 * PATCH_LANE_PX;     // stored pixels of one wave's span

// A one-wave workgroup owns a span of PATCH_WAVE_PX pixels of one patch slot, in the order the patch is stored (row-major, so
// that a patch narrower than a wave still fills it); a lane owns PATCH_LANE_PX consecutive ones.  The record's status rule and
// map are the same in every lane.  A lane's bytes are put together in registers.  ALIGNED (the patches' address and the bytes
// of a slot are multiples of 4): they are BPP whole dwords and stored as such, except in the lane that crosses the slot's end;
// everything else goes byte by byte.
template <int BPP, bool ALIGNED>
__global__ __launch_bounds__(64) void patch_kernel(PatchArgs a) {
    const int lane = threadIdx.x;
    const int k = blockIdx.y, f = blockIdx.z;
    int n = a.counts[f];
    n = n < a.slots ? n : a.slots;
    double M[9];
    const bool ok = k < n && patch_map(a.recs[(size_t)f * a.rec_stride + k], a.pw, a.ph, a.flags, M);
    if (a.status && blockIdx.x == 0 && lane == 0) a.status[(size_t)f * a.slots + k] = ok ? 1 : 0;
    if (!ok) return;   // (uniform)
    const int npx = a.pw * a.ph;
    const int q0 = blockIdx.x * PATCH_WAVE_PX + lane * PATCH_LANE_PX;
    if (q0 >= npx) return;
    const uint8_t* frame = a.frames + (size_t)f * a.frame_stride;
    uint8_t* out = a.patches + ((size_t)f * a.slots + k) * ((size_t)npx * BPP) + (size_t)q0 * BPP;
    int sy = q0 / a.pw, sx = q0 - sy * a.pw;   // the stored pixel's row and column
    unsigned q[BPP];
    OCVAR_UNROLL
    for (int j = 0; j < BPP; j++) q[j] = 0;
    OCVAR_UNROLL
    for (int i = 0; i < PATCH_LANE_PX; i++) {
        if (q0 + i < npx) {
            const int y = (a.flags & OCVAR_PATCH_FLIP_ROWS) ? a.ph - 1 - sy : sy;
            OCVAR_UNROLL
            for (int c = 0; c < BPP; c++) {
                const unsigned v = (unsigned)patch_sample(frame, a.W, a.H, a.row_stride, BPP, c, M, sx, y) & 255u;
                run_put(q, i * BPP + c, (int)v);
            }
        }
        if (++sx == a.pw) {
            sx = 0;
            sy++;
        }
    }
    if (ALIGNED && q0 + PATCH_LANE_PX <= npx) {
        run_store(q, out, true, 0);
    } else {   // (pixel by pixel: a lane's pixels end where the patch does)
        OCVAR_UNROLL
        for (int i = 0; i < PATCH_LANE_PX; i++)
            if (q0 + i < npx) {
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) out[i * BPP + c] = (uint8_t)run_byte(q, i * BPP + c);
            }
    }
}

template <int BPP>
static void launch_bpp(const PatchArgs& a, int n_frames, bool aligned, hipStream_t stream) {
    const dim3 grid((a.pw * a.ph + PATCH_WAVE_PX - 1) / PATCH_WAVE_PX, a.slots, n_frames);
    if (aligned)
        hipLaunchKernelGGL((patch_kernel<BPP, true>), grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((patch_kernel<BPP, false>), grid, dim3(64), 0, stream, a);
}

void launch_patches(const PatchArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || a.slots <= 0) return;
    const int bpp = format_bpp(format);
    const bool aligned = frames_dwords(a.patches, (long long)a.pw * a.ph * bpp, 0);   // (the "rows": the slots' patches)
    switch (bpp) {
        case 1: launch_bpp<1>(a, n_frames, aligned, stream); break;
        case 3: launch_bpp<3>(a, n_frames, aligned, stream); break;
        case 4: launch_bpp<4>(a, n_frames, aligned, stream); break;
        default: break;
    }
}

}  // namespace ocvar

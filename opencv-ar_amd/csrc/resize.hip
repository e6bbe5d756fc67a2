// resize.hip -- opt-in resizing of device-resident frames and scaling of marker records between two frame sizes
// (ocvar_hip_resize / ocvar_hip_scale_records).  The definition is resize_core.h's; its host build (tests/emul/resize_emul.cpp)
// gives these kernels' bytes.  All kernels are destination-oriented and pure streaming: no workspace and no stored map, every
// lane computes the taps of its pixels from the core's functions (double per column and row, cheap next to the loads).  The
// arguments travel by value; the kernels are templates of the bytes per pixel, the alignment and the rule, not of the sizes.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int RESIZE_LANE_PX = 8;                       // consecutive destination pixels of one row a lane owns: 8, 24 or 32 bytes
constexpr int RESIZE_WAVE_PX = 64 * RESIZE_LANE_PX;     // destination pixels of one wave's span

// Every kernel: a one-wave workgroup owns a span of RESIZE_WAVE_PX pixels of one destination row (blockIdx: span, row, frame), a
// lane RESIZE_LANE_PX consecutive ones, put together in registers.  A full lane stores them as 2 BPP whole dwords when the
// destination's address, row stride and frame stride are multiples of 4; the lane that crosses the row's end, and every lane
// when something is unaligned, stores byte by byte and touches nothing past its pixels.

// The K x K box (K 2 or 3: what "detect a 4K stream at 1080p or 720p" runs per frame).  A lane's source is contiguous, K rows of
// K RESIZE_LANE_PX BPP bytes, a multiple of 4: with ALIGNED (the source's address and strides multiples of 4 as well) a full lane
// loads them as whole dwords, else byte by byte and nothing outside its pixels' blocks.
template <int BPP, bool ALIGNED, int K>
__global__ __launch_bounds__(64) void resize_box_kernel(ResizeArgs a) {
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * RESIZE_LANE_PX;
    if (x0 >= a.dw) return;
    const int y = blockIdx.y;
    const int npx = a.dw - x0 < RESIZE_LANE_PX ? a.dw - x0 : RESIZE_LANE_PX;
    const bool dwords = ALIGNED && npx == RESIZE_LANE_PX;
    const uint8_t* in = a.src + (long long)blockIdx.z * a.src_frame_stride + (long long)y * K * a.src_row_stride + (long long)x0 * (K * BPP);
    int sum[RESIZE_LANE_PX * BPP];
    OCVAR_UNROLL
    for (int j = 0; j < RESIZE_LANE_PX * BPP; j++) sum[j] = 0;
    OCVAR_UNROLL
    for (int r = 0; r < K; r++) {
        unsigned w[2 * K * BPP];
        run_load(w, in + (long long)r * a.src_row_stride, dwords, npx * K * BPP);
        OCVAR_UNROLL
        for (int i = 0; i < RESIZE_LANE_PX; i++) {
            OCVAR_UNROLL
            for (int k = 0; k < K; k++) {
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) sum[i * BPP + c] += run_byte(w, (i * K + k) * BPP + c);
            }
        }
    }
    unsigned q[2 * BPP];
    OCVAR_UNROLL
    for (int j = 0; j < 2 * BPP; j++) q[j] = 0;
    OCVAR_UNROLL
    for (int j = 0; j < RESIZE_LANE_PX * BPP; j++) run_put(q, j, resize_box_value(sum[j], K, K, a.p.inv_area));
    uint8_t* out = a.dst + (long long)blockIdx.z * a.dst_frame_stride + (long long)y * a.dst_row_stride + (long long)x0 * BPP;
    run_store(q, out, dwords, npx * BPP);
}

// Every other rule gathers: the row's taps are the same for the whole workgroup, a pixel's column taps are computed once for its
// BPP bytes.  NEAREST reads 1 source pixel per pixel, LINEAR 4, BOX (any block but the two above) kx ky, TABLE up to 18 x 18.
// ALIGNED speaks of the destination alone.
template <int BPP, bool ALIGNED, int KIND>
__global__ __launch_bounds__(64) void resize_gather_kernel(ResizeArgs a) {
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * RESIZE_LANE_PX;
    if (x0 >= a.dw) return;
    const int y = blockIdx.y;
    const int npx = a.dw - x0 < RESIZE_LANE_PX ? a.dw - x0 : RESIZE_LANE_PX;
    const bool dwords = ALIGNED && npx == RESIZE_LANE_PX;
    const uint8_t* src = a.src + (long long)blockIdx.z * a.src_frame_stride;
    const long long rs = a.src_row_stride;
    const int ny = KIND == RESIZE_KIND_NEAREST ? resize_nearest_index(y, a.p.scale_y, a.sh) : 0;
    const ResizeLinearTap ly = KIND == RESIZE_KIND_LINEAR ? resize_linear_tap(y, a.p.scale_y, a.sh) : ResizeLinearTap{0, 0, 0, 0};
    const ResizeAreaSpan ty = KIND == RESIZE_KIND_TABLE ? resize_area_span(y, a.p.scale_y, a.sh) : ResizeAreaSpan{0, 0, false, false, 0.0f, 0.0f, 0.0f};
    unsigned q[2 * BPP];
    OCVAR_UNROLL
    for (int j = 0; j < 2 * BPP; j++) q[j] = 0;
    OCVAR_UNROLL
    for (int i = 0; i < RESIZE_LANE_PX; i++) {
        if (i < npx) {
            const int x = x0 + i;
            int px[BPP];
            if (KIND == RESIZE_KIND_NEAREST) {
                const uint8_t* p = src + (long long)ny * rs + (long long)resize_nearest_index(x, a.p.scale_x, a.sw) * BPP;
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) px[c] = p[c];
            } else if (KIND == RESIZE_KIND_LINEAR) {
                const ResizeLinearTap lx = resize_linear_tap(x, a.p.scale_x, a.sw);
                const uint8_t* r0 = src + (long long)ly.s0 * rs;
                const uint8_t* r1 = src + (long long)ly.s1 * rs;
                const long long c0 = (long long)lx.s0 * BPP, c1 = (long long)lx.s1 * BPP;
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) px[c] = resize_linear_value(r0[c0 + c], r0[c1 + c], r1[c0 + c], r1[c1 + c], lx, ly);
            } else if (KIND == RESIZE_KIND_BOX) {
                const uint8_t* p = src + (long long)y * a.p.ky * rs + (long long)x * a.p.kx * BPP;
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) px[c] = 0;
                for (int r = 0; r < a.p.ky; r++)
                    for (int k = 0; k < a.p.kx; k++) {
                        OCVAR_UNROLL
                        for (int c = 0; c < BPP; c++) px[c] += p[(long long)r * rs + k * BPP + c];
                    }
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) px[c] = resize_box_value(px[c], a.p.kx, a.p.ky, a.p.inv_area);
            } else {
                const ResizeAreaSpan tx = resize_area_span(x, a.p.scale_x, a.sw);
                const uint8_t* p = src + (long long)ty.first * rs + (long long)tx.first * BPP;
                float acc[BPP];
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) acc[c] = 0.0f;
                for (int r = 0; r < ty.n; r++) {
                    float row[BPP];
                    OCVAR_UNROLL
                    for (int c = 0; c < BPP; c++) row[c] = 0.0f;
                    for (int k = 0; k < tx.n; k++) {
                        const float alpha = resize_area_weight(tx, k);
                        OCVAR_UNROLL
                        for (int c = 0; c < BPP; c++) row[c] += (float)p[(long long)r * rs + k * BPP + c] * alpha;
                    }
                    const float beta = resize_area_weight(ty, r);
                    OCVAR_UNROLL
                    for (int c = 0; c < BPP; c++) acc[c] += beta * row[c];
                }
                OCVAR_UNROLL
                for (int c = 0; c < BPP; c++) px[c] = resize_rn_even_sat_u8(acc[c]);
            }
            OCVAR_UNROLL
            for (int c = 0; c < BPP; c++) run_put(q, i * BPP + c, px[c] & 255);
        }
    }
    uint8_t* out = a.dst + (long long)blockIdx.z * a.dst_frame_stride + (long long)y * a.dst_row_stride + (long long)x0 * BPP;
    run_store(q, out, dwords, npx * BPP);
}

template <int BPP, bool ALIGNED>
static void launch_aligned(const ResizeArgs& a, const dim3& grid, hipStream_t stream) {
    const bool square = a.p.kind == RESIZE_KIND_BOX && a.p.kx == a.p.ky;
    if (square && a.p.kx == 2) hipLaunchKernelGGL((resize_box_kernel<BPP, ALIGNED, 2>), grid, dim3(64), 0, stream, a);
    else if (square && a.p.kx == 3) hipLaunchKernelGGL((resize_box_kernel<BPP, ALIGNED, 3>), grid, dim3(64), 0, stream, a);
    else if (a.p.kind == RESIZE_KIND_BOX) hipLaunchKernelGGL((resize_gather_kernel<BPP, ALIGNED, RESIZE_KIND_BOX>), grid, dim3(64), 0, stream, a);
    else if (a.p.kind == RESIZE_KIND_NEAREST) hipLaunchKernelGGL((resize_gather_kernel<BPP, ALIGNED, RESIZE_KIND_NEAREST>), grid, dim3(64), 0, stream, a);
    else if (a.p.kind == RESIZE_KIND_LINEAR) hipLaunchKernelGGL((resize_gather_kernel<BPP, ALIGNED, RESIZE_KIND_LINEAR>), grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((resize_gather_kernel<BPP, ALIGNED, RESIZE_KIND_TABLE>), grid, dim3(64), 0, stream, a);
}

template <int BPP>
static void launch_bpp(const ResizeArgs& a, int n_frames, hipStream_t stream) {
    const dim3 grid((a.dw + RESIZE_WAVE_PX - 1) / RESIZE_WAVE_PX, a.dh, n_frames);
    // (the two box kernels load whole dwords too; the gathering ones read bytes wherever they lie)
    const bool box = a.p.kind == RESIZE_KIND_BOX && a.p.kx == a.p.ky && (a.p.kx == 2 || a.p.kx == 3);
    if (frames_dwords(a.dst, a.dst_row_stride, a.dst_frame_stride) && (!box || frames_dwords(a.src, a.src_row_stride, a.src_frame_stride))) launch_aligned<BPP, true>(a, grid, stream);
    else launch_aligned<BPP, false>(a, grid, stream);
}

void launch_resize(const ResizeArgs& a, int n_frames, int format, hipStream_t stream) {
    if (n_frames <= 0 || a.sw <= 0 || a.sh <= 0 || a.dw <= 0 || a.dh <= 0) return;
    switch (format_bpp(format)) {
        case 1: launch_bpp<1>(a, n_frames, stream); break;
        case 3: launch_bpp<3>(a, n_frames, stream); break;
        case 4: launch_bpp<4>(a, n_frames, stream); break;
        default: break;
    }
}

// One lane per record slot k < min(count, slots) of every frame (blockIdx: 64 slots, frame); the other slots are not written.
// A lane reads its record before it writes it, so out may be in.
__global__ __launch_bounds__(64) void scale_records_kernel(ScaleRecArgs a) {
    const int k = (int)blockIdx.x * 64 + (int)threadIdx.x, f = blockIdx.y;
    int n = a.counts[f];
    n = n < a.slots ? n : a.slots;
    if (k >= n) return;
    MarkerRec r = a.in[(size_t)f * a.slots + k];
    resize_record(r, a.sw, a.sh, a.dw, a.dh, a.flags, a.cam);
    a.out[(size_t)f * a.slots + k] = r;
}

void launch_scale_records(const ScaleRecArgs& a, int n_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.slots <= 0) return;
    hipLaunchKernelGGL(scale_records_kernel, dim3((a.slots + 63) / 64, n_frames), dim3(64), 0, stream, a);
}

}  // namespace ocvar

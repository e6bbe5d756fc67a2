// yuv.hip -- opt-in conversion of device-resident NV12, I420, YUYV and UYVY frames to and from the interleaved frame formats
// (ocvar_hip_yuv_to_frames / ocvar_hip_frames_to_yuv).  The definition is yuv_core.h's; its host build (tests/emul/yuv_emul.cpp)
// gives these kernels' bytes.  Both directions are pure streaming, 1.5 or 2 bytes per pixel on one side and 1, 3 or 4 on the
// other, with about 17 integer operations per pixel; no workspace.  The coefficient table travels by value in the launch
// arguments; the kernels are templates of the bytes per pixel, the alignment and the chroma subsampling, not of the table.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int YUV_LANE_PX = 8;                      // consecutive pixels of a row a lane owns (of two rows in 4:2:0)
constexpr int YUV_WAVE_PX = 64 * YUV_LANE_PX;       // pixels of one wave's span

// bytes 0 2 of lo and 0 2 of hi; bytes 1 3 of lo and 1 3 of hi; the two interleaved again
OCVAR_D unsigned even_bytes(unsigned lo, unsigned hi) {
    return (lo & 0xffu) | ((lo >> 8) & 0xff00u) | ((hi & 0xffu) << 16) | ((hi << 8) & 0xff000000u);
}
OCVAR_D unsigned odd_bytes(unsigned lo, unsigned hi) { return even_bytes(lo >> 8, hi >> 8); }
// bytes (2 h, 2 h + 1) of e and of o as e o e o
OCVAR_D unsigned interleave_bytes(unsigned e, unsigned o, int h) {
    const unsigned a = e >> (16 * h), b = o >> (16 * h);
    return (a & 0xffu) | ((b & 0xffu) << 8) | ((a & 0xff00u) << 8) | ((b & 0xff00u) << 16);
}
// UYVY <-> YUYV: the bytes of every halfword exchanged
OCVAR_D unsigned swap_halfword_bytes(unsigned w) { return ((w >> 8) & 0x00ff00ffu) | ((w << 8) & 0xff00ff00u); }

// A one-wave workgroup owns a span of YUV_WAVE_PX pixels of one row (4:2:2) or of a pair of rows (S420), blockIdx: span, row or
// row pair, frame; a lane owns YUV_LANE_PX consecutive ones of each row, so that in 4:2:0 every chroma pair is loaded once and
// serves both rows.  ALIGNED (every plane address, pitch, row stride and frame stride of both sides is a multiple of 4): a lane
// with all its pixels inside the row loads and stores whole dwords -- 8 bytes of Y per row, 8 of chroma (16 of a packed row) and
// 8 BPP of pixels per row; the lane that crosses the row's end, and every lane when something is unaligned, goes byte by byte
// and touches nothing past its pixels (widths are even: such a lane has 2, 4 or 6 pixels).
template <int BPP, bool ALIGNED, bool S420>
__global__ __launch_bounds__(64) void yuv_to_frames_kernel(YuvArgs a) {
    constexpr int ROWS = S420 ? 2 : 1;
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * YUV_LANE_PX;
    if (x0 >= a.W) return;
    const int y0 = (int)blockIdx.y * ROWS;
    const int npx = a.W - x0 < YUV_LANE_PX ? a.W - x0 : YUV_LANE_PX;
    const bool dwords = ALIGNED && npx == YUV_LANE_PX;
    const long long fo = (long long)blockIdx.z * a.yuv_frame_stride;
    unsigned yq[ROWS][2], uq[1], vq[1];
    if (S420) {
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) run_load(yq[r], a.y + fo + (long long)(y0 + r) * a.y_pitch + x0, dwords, npx);
        const long long co = fo + (long long)blockIdx.y * a.c_pitch;
        if (a.layout == OCVAR_YUV_NV12) {
            unsigned w[2];
            run_load(w, a.c0 + co + x0, dwords, npx);
            uq[0] = even_bytes(w[0], w[1]);
            vq[0] = odd_bytes(w[0], w[1]);
        } else {
            run_load(uq, a.c0 + co + (x0 >> 1), dwords, npx >> 1);
            run_load(vq, a.c1 + co + (x0 >> 1), dwords, npx >> 1);
        }
    } else {
        unsigned w[4];
        run_load(w, a.y + fo + (long long)y0 * a.y_pitch + 2 * x0, dwords, 2 * npx);
        if (a.layout == OCVAR_YUV_UYVY) {
            OCVAR_UNROLL
            for (int j = 0; j < 4; j++) w[j] = swap_halfword_bytes(w[j]);
        }
        yq[0][0] = even_bytes(w[0], w[1]);
        yq[0][1] = even_bytes(w[2], w[3]);
        const unsigned c01 = odd_bytes(w[0], w[1]), c23 = odd_bytes(w[2], w[3]);   // U V U V of pairs 0 1 and of pairs 2 3
        uq[0] = even_bytes(c01, c23);
        vq[0] = odd_bytes(c01, c23);
    }
    const bool rgb = yuv_fmt_rgb(a.format);
    unsigned q[ROWS][2 * BPP];
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) {
        OCVAR_UNROLL
        for (int j = 0; j < 2 * BPP; j++) q[r][j] = 0;
    }
    OCVAR_UNROLL
    for (int j = 0; j < YUV_LANE_PX / 2; j++) {
        int t[3];
        yuv_terms(a.k, run_byte(uq, j), run_byte(vq, j), rgb, t);
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            OCVAR_UNROLL
            for (int d = 0; d < 2; d++) {
                const int i = 2 * j + d;
                const int y = yuv_y_term(a.k, run_byte(yq[r], i));
                const int p0 = yuv_channel(y, t[0]), p1 = yuv_channel(y, t[1]), p2 = yuv_channel(y, t[2]);
                if (BPP == 1) {
                    run_put(q[r], i, yuv_grey(p0, p1, p2));   // (never rgb: p0 p1 p2 are B G R)
                } else {
                    run_put(q[r], i * BPP, p0);
                    run_put(q[r], i * BPP + 1, p1);
                    run_put(q[r], i * BPP + 2, p2);
                    if (BPP == 4) run_put(q[r], i * BPP + 3, 255);
                }
            }
        }
    }
    uint8_t* out = a.pix + (long long)blockIdx.z * a.pix_frame_stride + (long long)y0 * a.pix_row_stride + (long long)x0 * BPP;
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) run_store(q[r], out + (long long)r * a.pix_row_stride, dwords, npx * BPP);
}

// The other direction with the same ownership: a lane reads its 8 pixels of one row or of two, writes their 8 Y bytes per row
// and the 4 chroma pairs of the 2 x 2 (S420) or 2 x 1 blocks.
template <int BPP, bool ALIGNED, bool S420>
__global__ __launch_bounds__(64) void frames_to_yuv_kernel(YuvArgs a) {
    constexpr int ROWS = S420 ? 2 : 1;
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * YUV_LANE_PX;
    if (x0 >= a.W) return;
    const int y0 = (int)blockIdx.y * ROWS;
    const int npx = a.W - x0 < YUV_LANE_PX ? a.W - x0 : YUV_LANE_PX;
    const bool dwords = ALIGNED && npx == YUV_LANE_PX;
    const long long fo = (long long)blockIdx.z * a.yuv_frame_stride;
    const uint8_t* in = a.pix + (long long)blockIdx.z * a.pix_frame_stride + (long long)y0 * a.pix_row_stride + (long long)x0 * BPP;
    unsigned q[ROWS][2 * BPP];
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) run_load(q[r], in + (long long)r * a.pix_row_stride, dwords, npx * BPP);
    const YuvCoef k = yuv_coef_in_memory_order(a.k, yuv_fmt_rgb(a.format));   // (uniform: scalar registers)
    unsigned yq[ROWS][2], uq[1] = {0}, vq[1] = {0};
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) yq[r][0] = yq[r][1] = 0;
    OCVAR_UNROLL
    for (int j = 0; j < YUV_LANE_PX / 2; j++) {
        int s0 = 0, s1 = 0, s2 = 0;
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            OCVAR_UNROLL
            for (int d = 0; d < 2; d++) {
                const int i = 2 * j + d;
                const int p0 = run_byte(q[r], i * BPP);
                const int p1 = BPP == 1 ? p0 : run_byte(q[r], i * BPP + (BPP == 1 ? 0 : 1));
                const int p2 = BPP == 1 ? p0 : run_byte(q[r], i * BPP + (BPP == 1 ? 0 : 2));
                run_put(yq[r], i, yuv_luma(k, p0, p1, p2));
                s0 += p0;
                s1 += p1;
                s2 += p2;
            }
        }
        int U, V;
        yuv_chroma(k, s0, s1, s2, ROWS, &U, &V);   // 2^ROWS pixels: 4 in 4:2:0, 2 in 4:2:2
        run_put(uq, j, U);
        run_put(vq, j, V);
    }
    if (S420) {
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) run_store(yq[r], a.y + fo + (long long)(y0 + r) * a.y_pitch + x0, dwords, npx);
        const long long co = fo + (long long)blockIdx.y * a.c_pitch;
        if (a.layout == OCVAR_YUV_NV12) {
            const unsigned w[2] = {interleave_bytes(uq[0], vq[0], 0), interleave_bytes(uq[0], vq[0], 1)};
            run_store(w, a.c0 + co + x0, dwords, npx);
        } else {
            run_store(uq, a.c0 + co + (x0 >> 1), dwords, npx >> 1);
            run_store(vq, a.c1 + co + (x0 >> 1), dwords, npx >> 1);
        }
    } else {
        const unsigned c01 = interleave_bytes(uq[0], vq[0], 0), c23 = interleave_bytes(uq[0], vq[0], 1);   // U V U V
        unsigned w[4] = {interleave_bytes(yq[0][0], c01, 0), interleave_bytes(yq[0][0], c01, 1), interleave_bytes(yq[0][1], c23, 0),
                         interleave_bytes(yq[0][1], c23, 1)};                                               // Y U Y V
        if (a.layout == OCVAR_YUV_UYVY) {
            OCVAR_UNROLL
            for (int j = 0; j < 4; j++) w[j] = swap_halfword_bytes(w[j]);
        }
        run_store(w, a.y + fo + (long long)y0 * a.y_pitch + 2 * x0, dwords, 2 * npx);
    }
}

template <int BPP, bool ALIGNED, bool S420>
static void launch_one(const YuvArgs& a, int n_frames, bool to_frames, hipStream_t stream) {
    const dim3 grid((a.W + YUV_WAVE_PX - 1) / YUV_WAVE_PX, S420 ? a.H / 2 : a.H, n_frames);
    if (to_frames)
        hipLaunchKernelGGL((yuv_to_frames_kernel<BPP, ALIGNED, S420>), grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((frames_to_yuv_kernel<BPP, ALIGNED, S420>), grid, dim3(64), 0, stream, a);
}

template <int BPP>
static void launch_bpp(const YuvArgs& a, int n_frames, bool to_frames, bool aligned, hipStream_t stream) {
    const bool s420 = yuv_is_420(a.layout);
    if (aligned && s420) launch_one<BPP, true, true>(a, n_frames, to_frames, stream);
    else if (aligned) launch_one<BPP, true, false>(a, n_frames, to_frames, stream);
    else if (s420) launch_one<BPP, false, true>(a, n_frames, to_frames, stream);
    else launch_one<BPP, false, false>(a, n_frames, to_frames, stream);
}

void launch_yuv(const YuvArgs& a, int n_frames, bool to_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.W <= 0 || a.H <= 0) return;
    bool aligned = frames_dwords(a.y, a.y_pitch, a.yuv_frame_stride) && frames_dwords(a.pix, a.pix_row_stride, a.pix_frame_stride);
    if (yuv_is_420(a.layout)) aligned = aligned && frames_dwords(a.c0, a.c_pitch, 0);
    if (a.layout == OCVAR_YUV_I420) aligned = aligned && frames_dwords(a.c1, 0, 0);
    switch (format_bpp(a.format)) {
        case 1: launch_bpp<1>(a, n_frames, to_frames, aligned, stream); break;
        case 3: launch_bpp<3>(a, n_frames, to_frames, aligned, stream); break;
        case 4: launch_bpp<4>(a, n_frames, to_frames, aligned, stream); break;
        default: break;
    }
}

}  // namespace ocvar

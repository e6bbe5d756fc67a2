// yuv_ex.hip -- opt-in conversion of device-resident YUV frames of every layout, range, matrix and depth of OcvarYuvFramesEx to
// and from the interleaved frame formats (ocvar_hip_yuv_to_frames_ex / ocvar_hip_frames_to_yuv_ex).  The definition is
// yuv_ex_core.h's; its host build (tests/emul/yuv_ex_emul.cpp) gives these kernels' bytes.  The ownership is yuv.hip's, whose
// kernels stay what they are: pure streaming, no workspace, the coefficient table (with its offsets and shifts) by value in the
// launch arguments.  The kernels are templates of the bytes per pixel, the alignment, the chroma subsampling and the sample
// width, not of the table, the range, the matrix, the depth or the order of U and V.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int YEX_LANE_PX = 8;                      // consecutive pixels of a row a lane owns (of two rows in 4:2:0)
constexpr int YEX_WAVE_PX = 64 * YEX_LANE_PX;       // pixels of one wave's span

// UYVY <-> YUYV: the bytes of every halfword exchanged
OCVAR_D unsigned swap_halfword_bytes(unsigned w) { return ((w >> 8) & 0x00ff00ffu) | ((w << 8) & 0xff00ff00u); }

// the chroma samples a lane holds: one per pixel in 4:4:4, one per pixel pair otherwise
template <int SUB>
constexpr int yex_chroma() { return SUB == YUV_SUB_444 ? YEX_LANE_PX : YEX_LANE_PX / 2; }

// A one-wave workgroup owns a span of YEX_WAVE_PX pixels of one row (4:2:2, 4:4:4) or of a pair of rows (4:2:0), blockIdx: span,
// row or row pair, frame; a lane owns YEX_LANE_PX consecutive ones of each row.  ALIGNED (every plane address, pitch, row stride
// and frame stride of both sides is a multiple of 4): a lane with all its pixels inside the row loads and stores whole dwords --
// per row 8 bytes of 8-bit Y or 16 of 16-bit Y (one wide load), 8 or 16 of chroma, 8 BPP of pixels; the lane that crosses the row's
// end, and every lane when something is unaligned, goes byte by byte (halfword by halfword for 16-bit samples) and touches nothing
// past its pixels.  WIDE: 16-bit samples (NV12 only: P010, P012, P016).
//
// The samples of the lane as numbers: Y[r][i] of pixel i of row r, U[j] V[j] of chroma sample j.
template <int SUB, bool WIDE>
OCVAR_D void yex_load_samples(const YuvExArgs& a, int x0, int y0, int npx, bool dwords, int (&Y)[SUB == YUV_SUB_420 ? 2 : 1][YEX_LANE_PX],
                              int (&U)[yex_chroma<SUB>()], int (&V)[yex_chroma<SUB>()]) {
    constexpr int ROWS = SUB == YUV_SUB_420 ? 2 : 1;
    const long long fo = (long long)blockIdx.z * a.yuv_frame_stride;
    if (WIDE) {
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            unsigned q[4];
            run_load_halves(q, a.y + fo + (long long)(y0 + r) * a.y_pitch + 2 * x0, dwords, npx);
            OCVAR_UNROLL
            for (int i = 0; i < YEX_LANE_PX; i++) Y[r][i] = run_half(q, i) >> a.k.word_shift;
        }
        unsigned w[4];
        run_load_halves(w, a.c0 + fo + (long long)blockIdx.y * a.c_pitch + 2 * x0, dwords, npx);
        OCVAR_UNROLL
        for (int j = 0; j < YEX_LANE_PX / 2; j++) {
            U[j] = run_half(w, 2 * j) >> a.k.word_shift;
            V[j] = run_half(w, 2 * j + 1) >> a.k.word_shift;
        }
    } else if (SUB == YUV_SUB_420) {
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            unsigned q[2];
            run_load(q, a.y + fo + (long long)(y0 + r) * a.y_pitch + x0, dwords, npx);
            OCVAR_UNROLL
            for (int i = 0; i < YEX_LANE_PX; i++) Y[r][i] = run_byte(q, i);
        }
        const long long co = fo + (long long)blockIdx.y * a.c_pitch;
        if (yuv_ex_semiplanar(a.layout)) {
            unsigned w[2];
            run_load(w, a.c0 + co + x0, dwords, npx);
            const int first = a.layout == OCVAR_YUV_NV21 ? 1 : 0;   // (uniform) where U lies in a pair
            OCVAR_UNROLL
            for (int j = 0; j < YEX_LANE_PX / 2; j++) {
                const int c0 = run_byte(w, 2 * j), c1 = run_byte(w, 2 * j + 1);
                U[j] = first ? c1 : c0;
                V[j] = first ? c0 : c1;
            }
        } else {
            unsigned uq[1], vq[1];
            run_load(uq, a.c0 + co + (x0 >> 1), dwords, npx >> 1);
            run_load(vq, a.c1 + co + (x0 >> 1), dwords, npx >> 1);
            OCVAR_UNROLL
            for (int j = 0; j < YEX_LANE_PX / 2; j++) {
                U[j] = run_byte(uq, j);
                V[j] = run_byte(vq, j);
            }
        }
    } else if (SUB == YUV_SUB_422) {
        unsigned w[4];
        run_load(w, a.y + fo + (long long)y0 * a.y_pitch + 2 * x0, dwords, 2 * npx);
        if (a.layout == OCVAR_YUV_UYVY) {   // (uniform) to Y U Y V
            OCVAR_UNROLL
            for (int j = 0; j < 4; j++) w[j] = swap_halfword_bytes(w[j]);
        }
        OCVAR_UNROLL
        for (int i = 0; i < YEX_LANE_PX; i++) Y[0][i] = run_byte(w, 2 * i);
        OCVAR_UNROLL
        for (int j = 0; j < YEX_LANE_PX / 2; j++) {
            U[j] = run_byte(w, 4 * j + 1);
            V[j] = run_byte(w, 4 * j + 3);
        }
    } else {
        unsigned yq[2], uq[2], vq[2];
        run_load(yq, a.y + fo + (long long)y0 * a.y_pitch + x0, dwords, npx);
        const long long co = fo + (long long)y0 * a.c_pitch + x0;
        run_load(uq, a.c0 + co, dwords, npx);
        run_load(vq, a.c1 + co, dwords, npx);
        OCVAR_UNROLL
        for (int i = 0; i < YEX_LANE_PX; i++) {
            Y[0][i] = run_byte(yq, i);
            U[i] = run_byte(uq, i);
            V[i] = run_byte(vq, i);
        }
    }
}

template <int BPP, bool ALIGNED, int SUB, bool WIDE>
__global__ __launch_bounds__(64) void yuv_ex_to_frames_kernel(YuvExArgs a) {
    constexpr int ROWS = SUB == YUV_SUB_420 ? 2 : 1;
    constexpr int PER = SUB == YUV_SUB_444 ? 1 : 2;   // pixels of a row that share a chroma sample
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * YEX_LANE_PX;
    if (x0 >= a.W) return;
    const int y0 = (int)blockIdx.y * ROWS;
    const int npx = a.W - x0 < YEX_LANE_PX ? a.W - x0 : YEX_LANE_PX;
    const bool dwords = ALIGNED && npx == YEX_LANE_PX;
    int Y[ROWS][YEX_LANE_PX], U[yex_chroma<SUB>()], V[yex_chroma<SUB>()];
    yex_load_samples<SUB, WIDE>(a, x0, y0, npx, dwords, Y, U, V);
    const bool rgb = yuv_fmt_rgb(a.format);
    unsigned q[ROWS][2 * BPP];
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) {
        OCVAR_UNROLL
        for (int j = 0; j < 2 * BPP; j++) q[r][j] = 0;
    }
    OCVAR_UNROLL
    for (int j = 0; j < yex_chroma<SUB>(); j++) {
        int t[3];
        yuv_ex_terms(a.k, U[j], V[j], rgb, t);
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            OCVAR_UNROLL
            for (int d = 0; d < PER; d++) {
                const int i = PER * j + d;
                const int y = yuv_ex_y_term(a.k, Y[r][i]);
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

// The other direction with the same ownership: a lane reads its 8 pixels of one row or of two, writes their 8 Y samples per row
// and the chroma samples of the 2 x 2, 2 x 1 or single-pixel blocks.
template <int BPP, bool ALIGNED, int SUB, bool WIDE>
__global__ __launch_bounds__(64) void yuv_ex_from_frames_kernel(YuvExArgs a) {
    constexpr int ROWS = SUB == YUV_SUB_420 ? 2 : 1;
    constexpr int PER = SUB == YUV_SUB_444 ? 1 : 2;
    constexpr int NC = yex_chroma<SUB>();
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * YEX_LANE_PX;
    if (x0 >= a.W) return;
    const int y0 = (int)blockIdx.y * ROWS;
    const int npx = a.W - x0 < YEX_LANE_PX ? a.W - x0 : YEX_LANE_PX;
    const bool dwords = ALIGNED && npx == YEX_LANE_PX;
    const long long fo = (long long)blockIdx.z * a.yuv_frame_stride;
    const uint8_t* in = a.pix + (long long)blockIdx.z * a.pix_frame_stride + (long long)y0 * a.pix_row_stride + (long long)x0 * BPP;
    unsigned q[ROWS][2 * BPP];
    OCVAR_UNROLL
    for (int r = 0; r < ROWS; r++) run_load(q[r], in + (long long)r * a.pix_row_stride, dwords, npx * BPP);
    const YuvCoefEx k = yuv_ex_coef_in_memory_order(a.k, yuv_fmt_rgb(a.format));   // (uniform: scalar registers)
    int Y[ROWS][YEX_LANE_PX], U[NC], V[NC];
    OCVAR_UNROLL
    for (int j = 0; j < NC; j++) {
        int s0 = 0, s1 = 0, s2 = 0;
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            OCVAR_UNROLL
            for (int d = 0; d < PER; d++) {
                const int i = PER * j + d;
                const int p0 = run_byte(q[r], i * BPP);
                const int p1 = BPP == 1 ? p0 : run_byte(q[r], i * BPP + (BPP == 1 ? 0 : 1));
                const int p2 = BPP == 1 ? p0 : run_byte(q[r], i * BPP + (BPP == 1 ? 0 : 2));
                Y[r][i] = yuv_ex_luma(k, p0, p1, p2);
                s0 += p0;
                s1 += p1;
                s2 += p2;
            }
        }
        yuv_ex_chroma(k, s0, s1, s2, 2 - SUB, &U[j], &V[j]);   // 4, 2 or 1 pixels
    }
    if (WIDE) {
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            unsigned yq[4] = {0, 0, 0, 0};
            OCVAR_UNROLL
            for (int i = 0; i < YEX_LANE_PX; i++) run_put_half(yq, i, Y[r][i] << k.word_shift);
            run_store_halves(yq, a.y + fo + (long long)(y0 + r) * a.y_pitch + 2 * x0, dwords, npx);
        }
        unsigned w[4] = {0, 0, 0, 0};
        OCVAR_UNROLL
        for (int j = 0; j < NC; j++) {
            run_put_half(w, 2 * j, U[j] << k.word_shift);
            run_put_half(w, 2 * j + 1, V[j] << k.word_shift);
        }
        run_store_halves(w, a.c0 + fo + (long long)blockIdx.y * a.c_pitch + 2 * x0, dwords, npx);
    } else if (SUB == YUV_SUB_420) {
        OCVAR_UNROLL
        for (int r = 0; r < ROWS; r++) {
            unsigned yq[2] = {0, 0};
            OCVAR_UNROLL
            for (int i = 0; i < YEX_LANE_PX; i++) run_put(yq, i, Y[r][i]);
            run_store(yq, a.y + fo + (long long)(y0 + r) * a.y_pitch + x0, dwords, npx);
        }
        const long long co = fo + (long long)blockIdx.y * a.c_pitch;
        if (yuv_ex_semiplanar(a.layout)) {
            const int first = a.layout == OCVAR_YUV_NV21 ? 1 : 0;
            unsigned w[2] = {0, 0};
            OCVAR_UNROLL
            for (int j = 0; j < NC; j++) {
                run_put(w, 2 * j, first ? V[j] : U[j]);
                run_put(w, 2 * j + 1, first ? U[j] : V[j]);
            }
            run_store(w, a.c0 + co + x0, dwords, npx);
        } else {
            unsigned uq[1] = {0}, vq[1] = {0};
            OCVAR_UNROLL
            for (int j = 0; j < NC; j++) {
                run_put(uq, j, U[j]);
                run_put(vq, j, V[j]);
            }
            run_store(uq, a.c0 + co + (x0 >> 1), dwords, npx >> 1);
            run_store(vq, a.c1 + co + (x0 >> 1), dwords, npx >> 1);
        }
    } else if (SUB == YUV_SUB_422) {
        unsigned w[4] = {0, 0, 0, 0};   // as Y U Y V; UYVY: the bytes of every halfword exchanged
        OCVAR_UNROLL
        for (int j = 0; j < NC; j++) {
            run_put(w, 4 * j, Y[0][2 * j]);
            run_put(w, 4 * j + 1, U[j]);
            run_put(w, 4 * j + 2, Y[0][2 * j + 1]);
            run_put(w, 4 * j + 3, V[j]);
        }
        if (a.layout == OCVAR_YUV_UYVY) {
            OCVAR_UNROLL
            for (int j = 0; j < 4; j++) w[j] = swap_halfword_bytes(w[j]);
        }
        run_store(w, a.y + fo + (long long)y0 * a.y_pitch + 2 * x0, dwords, 2 * npx);
    } else {
        unsigned yq[2] = {0, 0}, uq[2] = {0, 0}, vq[2] = {0, 0};
        OCVAR_UNROLL
        for (int i = 0; i < YEX_LANE_PX; i++) {
            run_put(yq, i, Y[0][i]);
            run_put(uq, i, U[i]);
            run_put(vq, i, V[i]);
        }
        run_store(yq, a.y + fo + (long long)y0 * a.y_pitch + x0, dwords, npx);
        const long long co = fo + (long long)y0 * a.c_pitch + x0;
        run_store(uq, a.c0 + co, dwords, npx);
        run_store(vq, a.c1 + co, dwords, npx);
    }
}

template <int BPP, bool ALIGNED, int SUB, bool WIDE>
static void launch_one(const YuvExArgs& a, int n_frames, bool to_frames, hipStream_t stream) {
    const dim3 grid((a.W + YEX_WAVE_PX - 1) / YEX_WAVE_PX, SUB == YUV_SUB_420 ? a.H / 2 : a.H, n_frames);
    if (to_frames)
        hipLaunchKernelGGL((yuv_ex_to_frames_kernel<BPP, ALIGNED, SUB, WIDE>), grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((yuv_ex_from_frames_kernel<BPP, ALIGNED, SUB, WIDE>), grid, dim3(64), 0, stream, a);
}

template <int BPP, bool ALIGNED>
static void launch_sub(const YuvExArgs& a, int n_frames, bool to_frames, hipStream_t stream) {
    const int sub = yuv_ex_sub(a.layout);
    if (a.sample_bytes == 2) launch_one<BPP, ALIGNED, YUV_SUB_420, true>(a, n_frames, to_frames, stream);
    else if (sub == YUV_SUB_420) launch_one<BPP, ALIGNED, YUV_SUB_420, false>(a, n_frames, to_frames, stream);
    else if (sub == YUV_SUB_422) launch_one<BPP, ALIGNED, YUV_SUB_422, false>(a, n_frames, to_frames, stream);
    else launch_one<BPP, ALIGNED, YUV_SUB_444, false>(a, n_frames, to_frames, stream);
}

template <int BPP>
static void launch_bpp(const YuvExArgs& a, int n_frames, bool to_frames, bool aligned, hipStream_t stream) {
    if (aligned) launch_sub<BPP, true>(a, n_frames, to_frames, stream);
    else launch_sub<BPP, false>(a, n_frames, to_frames, stream);
}

void launch_yuv_ex(const YuvExArgs& a, int n_frames, bool to_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.W <= 0 || a.H <= 0) return;
    if (a.sample_bytes == 2 && a.layout != OCVAR_YUV_NV12) return;   // (refused before: 16-bit samples come as NV12 alone)
    bool aligned = frames_dwords(a.y, a.y_pitch, a.yuv_frame_stride) && frames_dwords(a.pix, a.pix_row_stride, a.pix_frame_stride);
    if (yuv_ex_sub(a.layout) != YUV_SUB_422) aligned = aligned && frames_dwords(a.c0, a.c_pitch, 0);
    if (a.layout == OCVAR_YUV_I420 || a.layout == OCVAR_YUV_I444) aligned = aligned && frames_dwords(a.c1, 0, 0);
    switch (format_bpp(a.format)) {
        case 1: launch_bpp<1>(a, n_frames, to_frames, aligned, stream); break;
        case 3: launch_bpp<3>(a, n_frames, to_frames, aligned, stream); break;
        case 4: launch_bpp<4>(a, n_frames, to_frames, aligned, stream); break;
        default: break;
    }
}

}  // namespace ocvar

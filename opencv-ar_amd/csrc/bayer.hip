// bayer.hip -- opt-in demosaic of device-resident raw Bayer frames into the interleaved frame formats (ocvar_hip_bayer_to_frames).
// The definition is bayer_core.h's; its host build (tests/emul/bayer_emul.cpp) gives these kernels' bytes, and the arithmetic of a
// lane (bayer_core.h: bayer_row_quads, bayer_pair) is the same source on both sides.  A 3 x 3 stencil on 1 or 2 bytes per pixel in,
// 1, 3 or 4 out; no workspace, no LDS.  Pattern, bits, black level and gains travel by value in the launch arguments and are
// wave-uniform; the kernels are templates of the bytes per destination pixel, the sample width and the alignment.
#include "kernels.h"
#include "lane_run.h"

namespace ocvar {

constexpr int BAYER_WAVE_PX = 64 * BAYER_LANE_PX;   // pixels of one wave's span

// The lane's ten raw samples of the source row at `row`: its own eight as whole dwords when `dwords`, the halo sample on either
// side (and all ten otherwise) one by one at the columns col, which the caller reflected into the row.
template <int SB>
OCVAR_D void bayer_row_samples(const uint8_t* row, int x0, bool dwords, const int (&col)[10], unsigned sample_mask, int (&t)[10]) {
    if (dwords) {
        unsigned w[2 * SB];
        run_load(w, row + (long long)x0 * SB, true, 8 * SB);
        OCVAR_UNROLL
        for (int i = 0; i < 8; i++) t[i + 1] = SB == 1 ? run_byte(w, i) : (int)((w[i >> 1] >> (16 * (i & 1))) & sample_mask);
        OCVAR_UNROLL
        for (int k = 0; k < 10; k += 9)
            t[k] = SB == 1 ? (int)row[col[k]] : (int)(*reinterpret_cast<const unsigned short*>(row + 2 * col[k]) & sample_mask);
    } else {
        OCVAR_UNROLL
        for (int k = 0; k < 10; k++)
            t[k] = SB == 1 ? (int)row[col[k]] : (int)(((unsigned)row[2 * col[k]] | ((unsigned)row[2 * col[k] + 1] << 8)) & sample_mask);
    }
}

// A one-wave workgroup owns a span of BAYER_WAVE_PX pixels of a strip of a.pairs even-aligned row pairs, blockIdx: span, strip,
// frame; a lane owns BAYER_LANE_PX consecutive pixels of each row, so the four Bayer phases are fixed positions of its run, and
// marches down the strip with the quads of four source rows in registers: the two rows below a pair are the two above the next,
// so inside a strip every source row is loaded, unpacked and balanced once (the rows at a strip's ends once more by the
// neighbouring strip, from L2).  A row is the lane's own 8 samples and one halo sample on either side, which the neighbouring lane
// loads as its own and L1 serves.  ALIGNED (every address, pitch and frame stride of both sides is a multiple of 4): a lane with
// all its pixels inside the row loads and stores whole dwords; the lane that crosses the row's end, and every lane when something
// is unaligned, goes sample by sample and byte by byte and touches nothing past its pixels.  Halo samples, the samples of a
// row-crossing lane and the rows around the frame are reflected (and, where no pixel of the lane needs them, clamped into the
// frame): no address outside the source's samples is formed.
template <int BPP, int SB, bool ALIGNED>
__global__ __launch_bounds__(64) void bayer_to_frames_kernel(BayerArgs a) {
    constexpr bool PACK = SB == 1;
    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * BAYER_LANE_PX;
    if (x0 >= a.W) return;
    const int npx = a.W - x0 < BAYER_LANE_PX ? a.W - x0 : BAYER_LANE_PX;
    const bool dwords = ALIGNED && npx == BAYER_LANE_PX;
    const uint8_t* frame = a.src + (long long)blockIdx.z * a.src_frame_stride;
    const unsigned sample_mask = (1u << a.p.bits) - 1u;
    const bool rgb = yuv_fmt_rgb(a.format);
    int col[10];
    OCVAR_UNROLL
    for (int k = 0; k < 10; k++) {
        const int x = bayer_reflect(x0 + k - 1 > a.W ? a.W : x0 + k - 1, a.W);   // (-1 .. W reflect; beyond W nothing is needed)
        col[k] = x < 0 ? 0 : x;
    }
    // row y (-1 .. H + 1; H + 1 is needed by no pixel) of the frame as the quads of a row of parity `parity`
    auto quads_of = [&](int y, int parity) {
        int yr = bayer_reflect(y > a.H ? a.H : y, a.H);
        yr = yr < 0 ? 0 : yr;
        int t[10];
        bayer_row_samples<SB>(frame + (long long)yr * a.src_pitch, x0, dwords, col, sample_mask, t);
        return bayer_row_quads<PACK>(a.p, parity, t);
    };
    const int y_first = (int)blockIdx.y * a.pairs * 2;
    const int y_end = y_first + 2 * a.pairs < a.H ? y_first + 2 * a.pairs : a.H;
    BayerRowQuads<PACK> rows[4];
    rows[0] = quads_of(y_first - 1, 1);
    rows[1] = quads_of(y_first, 0);
    uint8_t* out = a.dst + (long long)blockIdx.z * a.dst_frame_stride + (long long)y_first * a.dst_pitch + (long long)x0 * BPP;
    for (int y0 = y_first; y0 < y_end; y0 += 2, out += 2 * a.dst_pitch) {
        rows[2] = quads_of(y0 + 1, 1);
        rows[3] = quads_of(y0 + 2, 0);
        unsigned q[2][2 * BPP];
        bayer_pair<BPP, PACK>(a.p, rgb, rows, q);
        run_store(q[0], out, dwords, npx * BPP);
        if (y0 + 1 < a.H) run_store(q[1], out + a.dst_pitch, dwords, npx * BPP);
        rows[0] = rows[2];
        rows[1] = rows[3];
    }
}

template <int BPP, int SB>
static void launch_bpp(const BayerArgs& a, int n_frames, bool aligned, hipStream_t stream) {
    const int pairs = (a.H + 1) / 2;
    const dim3 grid((a.W + BAYER_WAVE_PX - 1) / BAYER_WAVE_PX, (pairs + a.pairs - 1) / a.pairs, n_frames);
    if (aligned)
        hipLaunchKernelGGL((bayer_to_frames_kernel<BPP, SB, true>), grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL((bayer_to_frames_kernel<BPP, SB, false>), grid, dim3(64), 0, stream, a);
}

template <int SB>
static void launch_sb(const BayerArgs& a, int n_frames, bool aligned, hipStream_t stream) {
    switch (format_bpp(a.format)) {
        case 1: launch_bpp<1, SB>(a, n_frames, aligned, stream); break;
        case 3: launch_bpp<3, SB>(a, n_frames, aligned, stream); break;
        case 4: launch_bpp<4, SB>(a, n_frames, aligned, stream); break;
        default: break;
    }
}

void launch_bayer(const BayerArgs& a, int n_frames, hipStream_t stream) {
    if (n_frames <= 0 || a.W < 2 || a.H < 2 || a.pairs < 1) return;
    const bool aligned = frames_dwords(a.src, a.src_pitch, a.src_frame_stride) && frames_dwords(a.dst, a.dst_pitch, a.dst_frame_stride);
    if (bayer_sample_bytes(a.p.bits) == 1) launch_sb<1>(a, n_frames, aligned, stream);
    else launch_sb<2>(a, n_frames, aligned, stream);
}

}  // namespace ocvar

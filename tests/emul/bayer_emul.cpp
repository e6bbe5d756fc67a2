// bayer_emul.cpp -- host build of the Bayer demosaic core (opencv-ar_amd/csrc/bayer_core.h) for the bayer tests: the sequential
// reference bayer_to_frames_emul, which the kernels of bayer.hip must match byte for byte; bayer_lanes_emul, the same frames through
// bayer_row_quads and bayer_pair, the kernels' own arithmetic on packed halves, with the loads of their sample-by-sample path and
// their march down a strip of row pairs; and the formulas one by
// one.  With -DBAYER_EMUL_MAIN: a program that runs a sweep on heap blocks of exactly the bytes a conversion may touch, for a
// sanitizer build (g++ -fsanitize=address,undefined) run on its own.
#include "bayer_core.h"

using namespace ocvar;

static BayerArgs args_of(const uint8_t* src, long long src_pitch, long long src_frame_stride, uint8_t* dst, long long dst_pitch,
                         long long dst_frame_stride, int W, int H, int format, const OcvarBayerParams* params, int pairs = BAYER_PAIRS) {
    OcvarBayerParams p;
    bayer_default_params(&p);
    if (params) p = *params;
    return BayerArgs{src, dst, src_pitch, src_frame_stride, dst_pitch, dst_frame_stride, W, H, format, p, pairs};
}

// one lane of the kernel on one strip of a.pairs row pairs, with the loads of its sample-by-sample path and its march: the quads
// of the two rows below a pair are kept for the next
template <int BPP, bool PACK>
static void lane_emul(const BayerArgs& a, int f, int x0, int y_first) {
    const int npx = a.W - x0 < BAYER_LANE_PX ? a.W - x0 : BAYER_LANE_PX;
    const uint8_t* frame = a.src + (long long)f * a.src_frame_stride;
    auto quads_of = [&](int y, int parity) {
        const int yr = bayer_reflect(y > a.H ? a.H : y, a.H);
        int t[10];
        for (int k = 0; k < 10; k++) {
            const int x = bayer_reflect(x0 + k - 1 > a.W ? a.W : x0 + k - 1, a.W);
            t[k] = bayer_raw(frame + (long long)yr * a.src_pitch, x, a.p.bits);
        }
        return bayer_row_quads<PACK>(a.p, parity, t);
    };
    const int y_end = y_first + 2 * a.pairs < a.H ? y_first + 2 * a.pairs : a.H;
    BayerRowQuads<PACK> rows[4];
    rows[0] = quads_of(y_first - 1, 1);
    rows[1] = quads_of(y_first, 0);
    for (int y0 = y_first; y0 < y_end; y0 += 2) {
        rows[2] = quads_of(y0 + 1, 1);
        rows[3] = quads_of(y0 + 2, 0);
        unsigned q[2][2 * BPP];
        bayer_pair<BPP, PACK>(a.p, yuv_fmt_rgb(a.format), rows, q);
        uint8_t* out = a.dst + (long long)f * a.dst_frame_stride + (long long)y0 * a.dst_pitch + (long long)x0 * BPP;
        run_store(q[0], out, false, npx * BPP);
        if (y0 + 1 < a.H) run_store(q[1], out + a.dst_pitch, false, npx * BPP);
        rows[0] = rows[2];
        rows[1] = rows[3];
    }
}

template <int BPP>
static void lanes_emul(const BayerArgs& a, int f) {
    for (int y_first = 0; y_first < a.H; y_first += 2 * a.pairs)
        for (int x0 = 0; x0 < a.W; x0 += BAYER_LANE_PX) {
            if (a.p.bits == 8) lane_emul<BPP, true>(a, f, x0, y_first);
            else lane_emul<BPP, false>(a, f, x0, y_first);
        }
}

extern "C" {

// The kernels' arguments, field by field, and the number of frames (params NULL: the defaults).  Returns bayer_params_bad.
int bayer_to_frames_emul(const uint8_t* src, long long src_pitch, long long src_frame_stride, uint8_t* dst, long long dst_pitch,
                         long long dst_frame_stride, int W, int H, int format, int n_frames, const OcvarBayerParams* params) {
    const BayerArgs a = args_of(src, src_pitch, src_frame_stride, dst, dst_pitch, dst_frame_stride, W, H, format, params);
    if (const int bad = bayer_params_bad(a.p)) return bad;
    for (int f = 0; f < n_frames; f++) bayer_to_frame(a, f);
    return 0;
}

// The same through the kernels' lanes, which march down strips of `pairs` row pairs (1 .. BAYER_MAX_PAIRS).
int bayer_lanes_emul(const uint8_t* src, long long src_pitch, long long src_frame_stride, uint8_t* dst, long long dst_pitch,
                     long long dst_frame_stride, int W, int H, int format, int n_frames, const OcvarBayerParams* params, int pairs) {
    const BayerArgs a = args_of(src, src_pitch, src_frame_stride, dst, dst_pitch, dst_frame_stride, W, H, format, params, pairs);
    if (const int bad = bayer_params_bad(a.p)) return bad;
    if (pairs < 1 || pairs > BAYER_MAX_PAIRS) return -2;
    for (int f = 0; f < n_frames; f++) {
        switch (format_bpp(format)) {
            case 1: lanes_emul<1>(a, f); break;
            case 3: lanes_emul<3>(a, f); break;
            case 4: lanes_emul<4>(a, f); break;
            default: return -1;
        }
    }
    return 0;
}

// how many of one frame's channel values do not fit a byte before the cast (0)
int bayer_cut_emul(const uint8_t* src, long long src_pitch, int W, int H, const OcvarBayerParams* params) {
    const BayerArgs a = args_of(src, src_pitch, 0, nullptr, 0, 0, W, H, OCVAR_FMT_BGR, params);
    int cut = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int B, G, R;
            bayer_pixel(a, src, x, y, &B, &G, &R);
            cut += ((B | G | R) >> 8) ? 1 : 0;
        }
    return cut;
}

void bayer_default_params_emul(OcvarBayerParams* p) { bayer_default_params(p); }
int bayer_params_bad_emul(const OcvarBayerParams* p) { return bayer_params_bad(*p); }
int bayer_pattern_at_emul(int pattern, int x0, int y0) { return bayer_pattern_at(pattern, x0, y0); }
int bayer_colour_at_emul(int pattern, int x, int y) { return bayer_colour_at(pattern, x, y); }
int bayer_reflect_emul(int i, int n) { return bayer_reflect(i, n); }
int bayer_balance_emul(int s, int black, int gain, int bits) { return bayer_balance(s, black, gain, (1 << bits) - 1); }
int bayer_reduce_emul(int v, int bits) { return bayer_reduce(v, bits); }
int bayer_pairs_emul(int which) { return which ? BAYER_MAX_PAIRS : BAYER_PAIRS; }

}  // extern "C"

#if defined(BAYER_EMUL_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// One heap block per side, of exactly the bytes from its first to its last sample or pixel byte: a byte read or written outside is
// the sanitizer's to report.  Rows carry a padding and frames a gap, whose bytes must keep their fill.
struct Block {
    uint8_t* p;
    long long row_bytes, rows, pitch, frame_stride, size;
    Block(long long row_bytes_, long long rows_, long long pad, long long gap, int n) : row_bytes(row_bytes_), rows(rows_) {
        pitch = row_bytes + pad;
        frame_stride = pitch * rows + gap;
        size = (n - 1) * frame_stride + (rows - 1) * pitch + row_bytes;
        p = (uint8_t*)malloc((size_t)size);
        memset(p, 0xA5, (size_t)size);
    }
    ~Block() { free(p); }
    void fill(unsigned* seed, int n) {
        for (int f = 0; f < n; f++)
            for (long long r = 0; r < rows; r++)
                for (long long b = 0; b < row_bytes; b++) {
                    *seed = *seed * 1664525u + 1013904223u;
                    p[f * frame_stride + r * pitch + b] = (uint8_t)(*seed >> 24);
                }
    }
    bool padding_kept() const {
        for (long long o = 0; o < size; o++) {
            const long long in_frame = o % frame_stride;
            if ((in_frame >= pitch * rows || in_frame % pitch >= row_bytes) && p[o] != 0xA5) return false;
        }
        return true;
    }
};

static int sweep_case(int pattern, int bits, int format, int W, int H, int n) {
    const int bpp = format_bpp(format), sb = bayer_sample_bytes(bits);
    unsigned seed = (unsigned)(pattern * 131 + format * 17 + W * 3 + H + bits);
    Block src((long long)sb * W, H, 2, 6, n), dst((long long)bpp * W, H, 1, 7, n), lanes((long long)bpp * W, H, 1, 7, n);
    src.fill(&seed, n);
    const OcvarBayerParams p{pattern, bits, bits == 8 ? 3 : 65, 1500, 900, 16383};
    int bad = 0;
    bad += bayer_to_frames_emul(src.p, src.pitch, src.frame_stride, dst.p, dst.pitch, dst.frame_stride, W, H, format, n, &p) != 0;
    bad += bayer_lanes_emul(src.p, src.pitch, src.frame_stride, lanes.p, lanes.pitch, lanes.frame_stride, W, H, format, n, &p, 1 + (W + bits) % 3) != 0;
    if (!dst.padding_kept() || !lanes.padding_kept()) bad++;
    if (memcmp(dst.p, lanes.p, (size_t)dst.size)) bad++;
    if (bpp == 4)
        for (int f = 0; f < n; f++)
            for (int r = 0; r < H; r++)
                for (int x = 0; x < W; x++) bad += dst.p[f * dst.frame_stride + r * dst.pitch + 4 * x + 3] != 255;
    return bad;
}

int main() {
    static const int sizes[][2] = {{2, 2}, {2, 3}, {3, 2}, {3, 3}, {5, 4}, {9, 7}, {17, 6}, {513, 5}};
    static const int depths[] = {8, 10, 12, 16};
    int bad = 0, cases = 0;
    for (int pattern = OCVAR_BAYER_RGGB; pattern <= OCVAR_BAYER_BGGR; pattern++)
        for (int format = OCVAR_FMT_BGR; format <= OCVAR_FMT_GRAY; format++)
            for (const auto& s : sizes)
                for (int bits : depths) {
                    bad += sweep_case(pattern, bits, format, s[0], s[1], 2);
                    cases++;
                }
    printf("bayer_emul: %d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif

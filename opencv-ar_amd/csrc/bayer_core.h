// bayer_core.h -- raw Bayer mosaics, as a machine-vision camera (GigE, USB3, CSI) delivers them, demosaiced into the interleaved
// frame formats on frames that stay in device memory (opt-in: ocvar_hip_bayer_to_frames).  What such a camera leaves in device
// memory becomes what render, annotate, patches, warp and frames_to_yuv take.  The call stands for OpenCV's cvtColor with
// COLOR_Bayer*2BGR (and the RGB, four-channel and grey relatives) behind a black level and a white balance.  No counterpart in the
// reference, which converts nothing.
//
// Patterns are named by the colours of the top-left 2 x 2 block, row by row: OCVAR_BAYER_RGGB 0, GRBG 1, GBRG 2, BGGR 3.  (OpenCV
// names its constants by the SECOND row's 2 x 2: COLOR_BayerBG2BGR is RGGB here, BayerGB is GRBG, BayerGR is GBRG, BayerRG is
// BGGR.)  Bit 0 of the code shifts RGGB by one column, bit 1 by one row, so the pattern of a source rectangle whose origin is pixel
// (x0, y0) is pattern ^ (x0 & 1) ^ ((y0 & 1) << 1): bayer_pattern_at.  A rectangle is a pointer offset, as everywhere else.
//
// Samples.  bits = 8: one byte per sample.  bits = 9 .. 16: one little-endian 16-bit word per sample, right-aligned; the sample is
// word & (2^bits - 1).  MSB-aligned data is read with bits = 16.
//
// Everything is integer arithmetic, in four steps:
//   black level and white balance, on each sample with the gain of the sample's own colour (1024 = 1.0, 0 .. 16383):
//                     s' = min(2^bits - 1, (max(s - black, 0) * gain_c + 512) >> 10)
//                   (the defaults, black 0 and gains 1024, give s' = s through this formula: there is no other path)
//   interpolation   bilinear at full depth, on s' (OpenCV's COLOR_Bayer*2BGR rule in the interior):
//                     at an R or B site   own colour = the sample, G = (N + S + W + E + 2) >> 2,
//                                         the opposite colour = (NW + NE + SW + SE + 2) >> 2
//                     at a G site         G = the sample, the colour of the row's other sites = (W + E + 1) >> 1,
//                                         the colour of the column's other sites = (N + S + 1) >> 1
//   borders         a coordinate outside the frame is reflected without repeating the edge, -1 -> 1 and W -> W - 2, which keeps the
//                   colour phase: the same formulas hold on the border, and a mosaic of one colour gives that colour everywhere.
//                   Any width and height >= 2, odd ones included.
//   reduction       for bits > 8, v8 = min(255, (v + (1 << (bits - 9))) >> (bits - 8)); bits = 8: v8 = v.  Written as the clamp
//                   before the shift, as yuv_shift_clamp is and for its reason ("A packed instruction the compiler gets
//                   wrong").
// The largest intermediate is the white balance's product, 65535 * 16383 + 512 = 1073660417, below 2^30; the neighbour sums stay
// below 2^18 and the reduction's sum below 2^17 (tests/test_bayer_cpu.py runs the extremes).
//
// The border rule is the library's own.  No OpenCV exists where this library is built and tested, so parity with an OpenCV build is
// unpinned and not claimed, for the interior as for the border (as for yuv_core.h); the rule above is the definition.
//
// The target is any OCVAR_FMT_*.  BGRA and RGBA get byte 3 = 255, and GRAY gets the library's grey of the demosaiced colour,
// (1868 B + 9617 G + 4899 R + 8192) >> 14 (yuv_grey): detection on that plane is detection on the demosaiced BGR frame.
//
// The host build (tests/emul/bayer_emul.cpp) gives the bytes of the kernels (bayer.hip).  bayer_to_frame is the host reference,
// sequential, pixel by pixel; bayer_row_quads and bayer_pair are the arithmetic of one lane of the kernels (a run of 8 pixels of a row
// pair, on halves packed two to a register), which the host build also runs, so that the packed form is held to the sequential one without a device.
#pragma once
#include "hd.h"
#include "lane_run.h"
#include "ocvar_hip.h"
#include "yuv_core.h"

namespace ocvar {

constexpr int BAYER_MAX_GAIN = 16383;
constexpr int BAYER_LANE_PX = 8;   // consecutive pixels of each row of an even-aligned row pair a lane owns
constexpr int BAYER_PAIRS = 4, BAYER_MAX_PAIRS = 64;   // row pairs a lane marches down: the default, the most (OCVAR_TUNE_BAYER_PAIRS)

OCVAR_HD bool bayer_pattern_ok(int pattern) { return pattern >= OCVAR_BAYER_RGGB && pattern <= OCVAR_BAYER_BGGR; }
OCVAR_HD int bayer_pattern_at(int pattern, int x0, int y0) { return bayer_pattern_ok(pattern) ? (pattern ^ (x0 & 1) ^ ((y0 & 1) << 1)) : -1; }
OCVAR_HD int bayer_sample_bytes(int bits) { return bits > 8 ? 2 : 1; }

inline void bayer_default_params(OcvarBayerParams* p) { *p = OcvarBayerParams{OCVAR_BAYER_RGGB, 8, 0, 1024, 1024, 1024}; }
// 0: fine; 1 pattern, 2 bits, 3 black, 4 a gain
inline int bayer_params_bad(const OcvarBayerParams& p) {
    if (!bayer_pattern_ok(p.pattern)) return 1;
    if (p.bits < 8 || p.bits > 16) return 2;
    if (p.black < 0 || p.black > (1 << p.bits) - 1) return 3;
    if (p.gain_b < 0 || p.gain_b > BAYER_MAX_GAIN || p.gain_g < 0 || p.gain_g > BAYER_MAX_GAIN || p.gain_r < 0 || p.gain_r > BAYER_MAX_GAIN) return 4;
    return 0;
}

// The colour of site (x, y): 0 B, 1 G, 2 R.  In RGGB's own phase (xn, yn) = (0, 0) is R and (1, 1) is B.
OCVAR_HD int bayer_colour_at(int pattern, int x, int y) {
    const int xn = (x ^ pattern) & 1, yn = (y ^ (pattern >> 1)) & 1;
    return xn != yn ? 1 : (xn ? 0 : 2);
}
OCVAR_HD int bayer_gain_of(const OcvarBayerParams& p, int colour) { return colour == 0 ? p.gain_b : (colour == 1 ? p.gain_g : p.gain_r); }

// -1 -> 1, n -> n - 2 (n >= 2; i in -1 .. n)
OCVAR_HD int bayer_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// black level and white balance of one sample: both factors are below 2^24 (the 24-bit multiplier on the device), the product
// below 2^30.  On the device in unsigned arithmetic -- a saturating subtraction, a multiply-add, a shift and a minimum, four
// instructions -- where the signed form below cost the compiler eight; the same number for 0 <= s, black <= top < 2^16.
OCVAR_HD int bayer_balance(int s, int black, int gain, int top) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned v = (umul24(__builtin_elementwise_sub_sat((unsigned)s, (unsigned)black), (unsigned)gain) + 512u) >> 10;
    return (int)(v < (unsigned)top ? v : (unsigned)top);
#else
    const int v = (yuv_mul(s > black ? s - black : 0, gain) + 512) >> 10;
    return v < top ? v : top;
#endif
}

// v8 of an interpolated value: the clamp of v + half to 0 .. 2^bits - 1 before the shift, the same number as the clamp to 255
// after it (v >= 0)
OCVAR_HD int bayer_reduce(int v, int bits) {
    const int sh = bits - 8;
    const int s = v + ((1 << sh) >> 1), top = (256 << sh) - 1;
    return (s > top ? top : s) >> sh;
}

// One launch's arguments, all pointers in device memory: frame f's mosaic starts src_frame_stride bytes after frame f - 1's, rows
// src_pitch bytes apart; its pixels start dst_frame_stride after frame f - 1's, rows dst_pitch apart.
struct BayerArgs {
    const uint8_t* src;
    uint8_t* dst;
    long long src_pitch, src_frame_stride, dst_pitch, dst_frame_stride;
    int W, H, format;
    OcvarBayerParams p;
    int pairs;   // row pairs a lane of the kernels marches down (>= 1; the host reference does not look at it)
};

// sample x of the row at `row`, before the black level
OCVAR_HD int bayer_raw(const uint8_t* row, int x, int bits) {
    if (bits == 8) return row[x];
    return ((int)row[2 * x] | ((int)row[2 * x + 1] << 8)) & ((1 << bits) - 1);
}

// s' of site (x, y) of the frame at `frame`, x and y reflected
OCVAR_HD int bayer_site(const BayerArgs& a, const uint8_t* frame, int x, int y) {
    const int xr = bayer_reflect(x, a.W), yr = bayer_reflect(y, a.H);
    const int gain = bayer_gain_of(a.p, bayer_colour_at(a.p.pattern, xr, yr));
    return bayer_balance(bayer_raw(frame + (long long)yr * a.src_pitch, xr, a.p.bits), a.p.black, gain, (1 << a.p.bits) - 1);
}

// B G R of pixel (x, y), reduced to 8 bits
OCVAR_HD void bayer_pixel(const BayerArgs& a, const uint8_t* frame, int x, int y, int* B, int* G, int* R) {
    const int c = bayer_colour_at(a.p.pattern, x, y);
    const int own = bayer_site(a, frame, x, y);
    const int n = bayer_site(a, frame, x, y - 1), s = bayer_site(a, frame, x, y + 1);
    const int w = bayer_site(a, frame, x - 1, y), e = bayer_site(a, frame, x + 1, y);
    int v[3];
    if (c == 1) {
        const int row_colour = bayer_colour_at(a.p.pattern, x + 1, y);   // 0 or 2
        v[1] = own;
        v[row_colour] = (w + e + 1) >> 1;
        v[2 - row_colour] = (n + s + 1) >> 1;
    } else {
        const int d = bayer_site(a, frame, x - 1, y - 1) + bayer_site(a, frame, x + 1, y - 1) + bayer_site(a, frame, x - 1, y + 1) +
                      bayer_site(a, frame, x + 1, y + 1);
        v[c] = own;
        v[1] = (n + s + w + e + 2) >> 2;
        v[2 - c] = (d + 2) >> 2;
    }
    *B = bayer_reduce(v[0], a.p.bits);
    *G = bayer_reduce(v[1], a.p.bits);
    *R = bayer_reduce(v[2], a.p.bits);
}

// The host reference: frame f of the launch, sequentially.
inline void bayer_to_frame(const BayerArgs& a, int f) {
    const int bpp = format_bpp(a.format);
    const bool rgb = yuv_fmt_rgb(a.format);
    const uint8_t* frame = a.src + (long long)f * a.src_frame_stride;
    for (int y = 0; y < a.H; y++)
        for (int x = 0; x < a.W; x++) {
            int B, G, R;
            bayer_pixel(a, frame, x, y, &B, &G, &R);
            uint8_t* out = a.dst + (long long)f * a.dst_frame_stride + (long long)y * a.dst_pitch + (long long)x * bpp;
            for (int c = 0; c < bpp; c++) out[c] = (uint8_t)yuv_pixel_byte(bpp, rgb, c, B, G, R);
        }
}

// ---- one lane of the kernels -------------------------------------------------------------------------------------------------------
// A lane owns pixels x0 .. x0 + 7 (x0 a multiple of 8) of rows y0, y0 + 1 (y0 even), so the four Bayer phases sit at fixed
// positions of its run.  It holds samples x0 - 1 .. x0 + 8 of source rows y0 - 1 .. y0 + 2 (reflected).  The pixels of one row and one column parity are one kind of site, so the arithmetic runs on
// quads: the four values of a parity, PACK two to a register in 16-bit halves (8-bit samples: every sum stays below 2^16, and a
// plain 32-bit add is two 16-bit adds) or one to a register (16-bit samples, whose sums need 18 bits).
template <bool PACK>
struct BayerQuad {
    unsigned v[PACK ? 2 : 4];
};
template <bool PACK>
OCVAR_HD BayerQuad<PACK> bayer_quad(int a, int b, int c, int d) {
    if constexpr (PACK)
        return BayerQuad<PACK>{{(unsigned)a | ((unsigned)b << 16), (unsigned)c | ((unsigned)d << 16)}};
    else
        return BayerQuad<PACK>{{(unsigned)a, (unsigned)b, (unsigned)c, (unsigned)d}};
}
template <bool PACK>
OCVAR_HD int bayer_quad_get(const BayerQuad<PACK>& q, int k) {
    if constexpr (PACK)
        return (int)((q.v[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    else
        return (int)q.v[k];
}
template <bool PACK>
OCVAR_HD BayerQuad<PACK> bayer_quad_add(const BayerQuad<PACK>& a, const BayerQuad<PACK>& b) {
    BayerQuad<PACK> q;
    OCVAR_UNROLL
    for (int i = 0; i < (PACK ? 2 : 4); i++) q.v[i] = a.v[i] + b.v[i];
    return q;
}
// (a + half) >> K of every value: the shift of a packed register lets bits of the upper half into the lower, which the mask drops
template <bool PACK, int K>
OCVAR_HD BayerQuad<PACK> bayer_quad_round(const BayerQuad<PACK>& a) {
    constexpr unsigned half = PACK ? (unsigned)(1 << (K - 1)) * 0x10001u : (unsigned)(1 << (K - 1));
    constexpr unsigned mask = PACK ? (0xffffu >> K) * 0x10001u : 0xffffffffu;
    BayerQuad<PACK> q;
    OCVAR_UNROLL
    for (int i = 0; i < (PACK ? 2 : 4); i++) q.v[i] = ((a.v[i] + half) >> K) & mask;
    return q;
}

// bytes of b (selector digits 0 .. 3) and of a (4 .. 7), byte i of the result by digit i of sel from the right: v_perm_b32
OCVAR_HD unsigned bayer_bytes(unsigned a, unsigned b, unsigned sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(a, b, sel);
#else
    const unsigned long long ab = ((unsigned long long)a << 32) | b;
    unsigned r = 0;
    for (int i = 0; i < 4; i++) r |= (unsigned)((ab >> (8 * ((sel >> (8 * i)) & 7u))) & 255u) << (8 * i);
    return r;
#endif
}

// The bytes of eight pixels of three or four bytes from packed quads whose values fit a byte: f g t the first, second and third
// byte of the even pixels (fe ..: values of pixels 0 2 in [0], 4 6 in [1]) and of the odd pixels (fo ..: 1 3 and 5 7).  Seven
// instructions for twelve bytes (BPP 3), where byte-by-byte extraction and insertion takes two per byte.
template <int BPP>
OCVAR_HD void bayer_pack_pixels(const BayerQuad<true>& fe, const BayerQuad<true>& ge, const BayerQuad<true>& te, const BayerQuad<true>& fo,
                                const BayerQuad<true>& go, const BayerQuad<true>& to, unsigned (&q)[2 * BPP]) {
    OCVAR_UNROLL
    for (int h = 0; h < 2; h++) {   // pixels 4 h .. 4 h + 3: a b of the even quads, c d of the odd ones
        const unsigned xe = fe.v[h] | (ge.v[h] << 8);   // fa ga fb gb
        if (BPP == 3) {
            const unsigned ye = te.v[h] | (fo.v[h] << 8);   // ta fc tb fd
            const unsigned yo = go.v[h] | (to.v[h] << 8);   // gc tc gd td
            q[3 * h] = bayer_bytes(ye, xe, 0x05040100u);       // fa ga ta fc
            q[3 * h + 1] = bayer_bytes(xe, yo, 0x07060100u);   // gc tc fb gb
            q[3 * h + 2] = bayer_bytes(yo, ye, 0x07060302u);   // tb fd gd td
        } else {
            const unsigned xo = fo.v[h] | (go.v[h] << 8);       // fc gc fd gd
            const unsigned ze = te.v[h] | 0xff00ff00u, zo = to.v[h] | 0xff00ff00u;   // ta 255 tb 255; tc 255 td 255
            q[4 * h] = bayer_bytes(ze, xe, 0x05040100u);
            q[4 * h + 1] = bayer_bytes(zo, xo, 0x05040100u);
            q[4 * h + 2] = bayer_bytes(ze, xe, 0x07060302u);
            q[4 * h + 3] = bayer_bytes(zo, xo, 0x07060302u);
        }
    }
}

// a source row's samples by parity: e the lane's even pixels 0 2 4 6, o its odd pixels 1 3 5 7, and the sums of the two samples that
// flank each even pixel (fe: -1+1, 1+3, ..) and each odd pixel (fo: 0+2, 2+4, ..)
template <bool PACK>
struct BayerRowQuads {
    BayerQuad<PACK> e, o, fe, fo;
};

// A source row's quads from the lane's ten raw samples t (before the black level): t[k] is sample x0 + k - 1 of a row whose parity
// is row_parity (the reflection keeps both parities, so sample k has the column parity of k - 1).  Entries the caller could not load
// may hold anything as long as no pixel it stores needs them.
template <bool PACK>
OCVAR_D BayerRowQuads<PACK> bayer_row_quads(const OcvarBayerParams& p, int row_parity, const int (&t)[10]) {
    const int top = (1 << p.bits) - 1;
    const int g_even = bayer_gain_of(p, bayer_colour_at(p.pattern, 0, row_parity)), g_odd = bayer_gain_of(p, bayer_colour_at(p.pattern, 1, row_parity));
    int s[10];
    OCVAR_UNROLL
    for (int k = 0; k < 10; k++) s[k] = bayer_balance(t[k], p.black, (k & 1) ? g_even : g_odd, top);
    BayerRowQuads<PACK> row;
    row.e = bayer_quad<PACK>(s[1], s[3], s[5], s[7]);
    row.o = bayer_quad<PACK>(s[2], s[4], s[6], s[8]);
    row.fe = bayer_quad_add(bayer_quad<PACK>(s[0], s[2], s[4], s[6]), row.o);
    row.fo = bayer_quad_add(row.e, bayer_quad<PACK>(s[3], s[5], s[7], s[9]));
    return row;
}

// The lane's 2 x 8 pixels of the row pair y0, y0 + 1 from the quads of source rows y0 - 1 .. y0 + 2: q[r] is the run of row
// y0 + r's bytes in `format`.  (rows[2] and rows[3] are rows[0] and rows[1] of the next pair: a lane that marches down keeps them.)
template <int BPP, bool PACK>
OCVAR_D void bayer_pair(const OcvarBayerParams& p, bool rgb, const BayerRowQuads<PACK> (&rows)[4], unsigned (&q)[2][2 * BPP]) {
    OCVAR_UNROLL
    for (int r = 0; r < 2; r++) {
        const BayerRowQuads<PACK>&up = rows[r], &mid = rows[r + 1], &down = rows[r + 2];
        const int yn = (r ^ (p.pattern >> 1)) & 1;          // the row in RGGB's own phase: 0 a row of R and G, 1 of G and B
        const bool first_is_row = (yn == 1) != rgb;         // whether byte 0 (B, or R when rgb) is the colour of the row's sites
        OCVAR_UNROLL
        for (int j = 0; j < 2 * BPP; j++) q[r][j] = 0;
        BayerQuad<PACK> first[2], second[2], third[2];   // the pixels' bytes 0, 1 and 2, of the even pixels and of the odd ones
        OCVAR_UNROLL
        for (int par = 0; par < 2; par++) {
            const BayerQuad<PACK>& own = par ? mid.o : mid.e;
            const BayerQuad<PACK>& hs = par ? mid.fo : mid.fe;                                                         // W + E
            const BayerQuad<PACK> vs = par ? bayer_quad_add(up.o, down.o) : bayer_quad_add(up.e, down.e);              // N + S
            BayerQuad<PACK> v_row, v_g, v_col;   // the colour of the row's R or B sites, green, the colour of the other rows' sites
            if ((((par ^ p.pattern) & 1) == yn)) {   // an R or B site
                v_row = own;
                v_g = bayer_quad_round<PACK, 2>(bayer_quad_add(hs, vs));
                v_col = bayer_quad_round<PACK, 2>(par ? bayer_quad_add(up.fo, down.fo) : bayer_quad_add(up.fe, down.fe));
            } else {
                v_row = bayer_quad_round<PACK, 1>(hs);
                v_g = own;
                v_col = bayer_quad_round<PACK, 1>(vs);
            }
            if (p.bits > 8) {
                const unsigned half = (1u << (p.bits - 8)) >> 1, cut = (256u << (p.bits - 8)) - 1u;
                OCVAR_UNROLL
                for (int i = 0; i < (PACK ? 2 : 4); i++) {   // (PACK serves bits = 8 alone: the kernels never come here with it)
                    const unsigned s0 = v_row.v[i] + half, s1 = v_g.v[i] + half, s2 = v_col.v[i] + half;
                    v_row.v[i] = (s0 > cut ? cut : s0) >> (p.bits - 8);
                    v_g.v[i] = (s1 > cut ? cut : s1) >> (p.bits - 8);
                    v_col.v[i] = (s2 > cut ? cut : s2) >> (p.bits - 8);
                }
            }
            first[par] = first_is_row ? v_row : v_col;
            second[par] = v_g;
            third[par] = first_is_row ? v_col : v_row;
        }
        if constexpr (PACK && BPP != 1) {
            bayer_pack_pixels<BPP>(first[0], second[0], third[0], first[1], second[1], third[1], q[r]);
        } else {
            OCVAR_UNROLL
            for (int i = 0; i < 8; i++) {
                const int p0 = bayer_quad_get(first[i & 1], i >> 1), p1 = bayer_quad_get(second[i & 1], i >> 1), p2 = bayer_quad_get(third[i & 1], i >> 1);
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
}

}  // namespace ocvar

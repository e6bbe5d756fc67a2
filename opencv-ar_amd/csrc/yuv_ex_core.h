// yuv_ex_core.h -- YUV frames of every range, depth and layout the library takes (ocvar_hip_yuv_to_frames_ex /
// ocvar_hip_frames_to_yuv_ex) to and from the interleaved frame formats: what yuv_core.h defines for 8-bit limited-range NV12,
// I420, YUYV and UYVY, extended to NV21 and planar 4:4:4 (I444), to full range, to the BT.2020 matrix and to P010 / P012 / P016
// (NV12 in 16-bit little-endian words, the sample in the high bits).  The old entry points and yuv_core.h stay as they are: they
// are the 8-bit limited-range subset, and on every case both accept the two give the same bytes.  No counterpart in the reference.
//
// All integer, in yuv_core.h's 20-bit fixed point (YUV_SHIFT), floor shift with the rounding half, clamp before the shift.  With n
// the depth (8, 10, 12, 16), Y0 the luma offset and C the chroma centre of the table (limited: 16 << (n - 8), full: 0; C =
// 128 << (n - 8)), a sample s = word >> (16 - n) at n > 8 (the low bits are ignored on read and written as zero):
//   YUV to colour   u = U - C, v = V - C, y = max(Y - Y0, 0) * CY
//                     R = clamp255((y + 2^19 + CVR v) >> 20), G and B as in yuv_core.h
//                   The extra n - 8 bits of a sample are absorbed in the coefficient's scale: CY = round(2^20 * 255 / (219 * 2^(n-8)))
//                   and so on, so a coefficient of the 8-bit matrix holds 28 - n fractional bits (12 at 16 bits) and the shift is
//                   always 20.
//   colour to Y     Y = clampN((RY R + GY G + BY B + 2^(27-n) + (Y0 << (28 - n))) >> (28 - n)), clampN: to 0 .. 2^n - 1.  Limited
//                   range is an offset, not a clamp: Y is not held to 16 .. 235, as in yuv_core.h.
//   colour to U, V  from the channel sums over the 2^log2n pixels that share the sample (4:2:0: 4, 4:2:2: 2, 4:4:4: the pixel, 1):
//                     U = clampN((RU sR + GU sG + BU sB + (2^(27-n) << log2n) + (C << (28 - n + log2n))) >> (28 - n + log2n))
//                   The coefficients of this direction hold 20 fractional bits at every depth; the shift makes the depth.
// Y0 << (28 - n) is 16 << 20 or 0 and C << (28 - n) is 128 << 20 at every depth, and the clamp before the shift is to
// 0 .. 2^(28 + log2n) - 1 at every depth: the kernels need the shift alone.
//
// Operand sizes.  Every product is a 24-bit one (yuv_mul): a factor is a sample or a sample minus an offset (|.| < 2^16), a byte
// or a sum of four bytes (<= 1020), the other a coefficient below 2^23 (the largest, CUB of BT.2020 limited at 8 bits, is
// 2245829; tests/test_yuv_ex_cpu.py asserts the bound on every table).  Every sum fits an int:
//   YUV to colour   |sample| * |coefficient| <= 2^n * 2.15 * 2^(28 - n) = 2.15 * 2^28 per term with the 2.15 only for chroma, whose
//                   factor is below 2^(n-1): y <= 1.17 * 2^28, a chroma term <= 1.08 * 2^28, G's two chroma terms <= 0.6 * 2^28
//                   together; the largest sum is below 2.3 * 2^28 < 2^30, the smallest above -1.1 * 2^28
//   colour to Y     (RY + GY + BY) * 255 <= 2^20 * 255 plus 16 * 2^20 and the half: below 2^29
//   colour to U, V  |coefficient| <= 2^19, a sum of four bytes <= 1020: the coefficient terms lie within +-2^29, the bias is
//                   128 * 2^22 = 2^29: between 0 and 2^30
//
// Tables.  yuv_coef_ex(matrix, range, bits) returns YUV_COEF_BT601 / YUV_COEF_BT709 verbatim for 8 bits, limited range, BT.601 or
// BT.709; every other table is floor(x * 2^20 + 0.5) of the float64 matrix with Kr, Kb = (0.299, 0.114), (0.2126, 0.0722),
// (0.2627, 0.0593), Kg = 1 - Kr - Kb and the scales sy = 255 / (219 * 2^(n-8)), sc = 255 / (224 * 2^(n-8)) (limited) or sy = sc =
// 255 / (2^n - 1) (full):
//   cy = sy, cvr = 2 (1 - Kr) sc, cub = 2 (1 - Kb) sc, cug = -2 Kb (1 - Kb) / Kg sc, cvg = -2 Kr (1 - Kr) / Kg sc
//   ry gy by = Kr Kg Kb / (sy 2^(n-8)); ru gu bu = (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb) sc 2^(n-8)); rv gv bv = (1 - Kr, -Kg, -Kb) /
//   (2 (1 - Kr) sc 2^(n-8))
// BT.2020 is the matrix alone: no transfer function, no tone mapping.  The table travels by value in the launch arguments; the
// kernels do not know which range, matrix or depth they hold.
//
// Layouts.  yuv_core.h's four, and OCVAR_YUV_NV21 (NV12 with V first in the interleaved plane) and OCVAR_YUV_I444 (three planes of
// full resolution: Y at y, U at c0, V at c1, both chroma planes c_pitch apart; no subsampling, so odd widths and heights are
// taken).  Depths above 8 come with OCVAR_YUV_NV12 only (P010, P012, P016); pitches stay in bytes, and the plane addresses, the
// pitches and the frame stride of 16-bit samples are even.  The pixel side is yuv_core.h's, rule for rule.
//
// yuv_ex_check is everything the two entry points refuse, in the order they look; frame_ops.hip gives the reasons their texts.
// The host build (tests/emul/yuv_ex_emul.cpp) gives the bytes of the kernels (yuv_ex.hip).
#pragma once
#include <math.h>
#include "frames_core.h"
#include "yuv_core.h"

namespace ocvar {

struct YuvCoefEx {
    YuvCoef k;
    int y_off, c_mid;   // what YUV to colour takes off a luma and off a chroma sample
    int out_y_off;      // what colour to Y adds, in the sum's scale: y_off << out_shift
    int out_shift;      // colour to YUV: 28 - bits
    int word_shift;     // 16 - bits: sample = word >> word_shift (16-bit samples only)
};

OCVAR_HD bool yuv_ex_layout_ok(int layout) { return layout >= OCVAR_YUV_NV12 && layout <= OCVAR_YUV_I444; }
inline bool yuv_ex_matrix_ok(int matrix) { return matrix >= OCVAR_YUV_BT601 && matrix <= OCVAR_YUV_BT2020; }
inline bool yuv_ex_range_ok(int range) { return range == OCVAR_YUV_LIMITED || range == OCVAR_YUV_FULL; }
inline bool yuv_ex_bits_ok(int bits) { return bits == 8 || bits == 10 || bits == 12 || bits == 16; }
// chroma subsampling of a layout: 0 -- 4:2:0, 1 -- 4:2:2, 2 -- 4:4:4
enum { YUV_SUB_420 = 0, YUV_SUB_422 = 1, YUV_SUB_444 = 2 };
OCVAR_HD int yuv_ex_sub(int layout) {
    return layout == OCVAR_YUV_I444 ? YUV_SUB_444 : ((layout == OCVAR_YUV_YUYV || layout == OCVAR_YUV_UYVY) ? YUV_SUB_422 : YUV_SUB_420);
}
OCVAR_HD bool yuv_ex_semiplanar(int layout) { return layout == OCVAR_YUV_NV12 || layout == OCVAR_YUV_NV21; }

inline int yuv_ex_round(double x) { return (int)floor(x * 1048576.0 + 0.5); }

inline YuvCoefEx yuv_coef_ex(int matrix, int range, int bits) {
    const bool full = range == OCVAR_YUV_FULL;
    YuvCoefEx t;
    t.y_off = full ? 0 : 16 << (bits - 8);
    t.c_mid = 128 << (bits - 8);
    t.out_shift = YUV_SHIFT + 8 - bits;
    t.out_y_off = t.y_off << t.out_shift;
    t.word_shift = 16 - bits;
    if (bits == 8 && !full && yuv_matrix_ok(matrix)) {
        t.k = yuv_coef(matrix);
        return t;
    }
    const double kr = matrix == OCVAR_YUV_BT2020 ? 0.2627 : (matrix == OCVAR_YUV_BT709 ? 0.2126 : 0.299);
    const double kb = matrix == OCVAR_YUV_BT2020 ? 0.0593 : (matrix == OCVAR_YUV_BT709 ? 0.0722 : 0.114);
    const double kg = 1.0 - kr - kb;
    const double up = (double)(1 << (bits - 8));   // 2^(n-8)
    const double sy = full ? 255.0 / (double)((1 << bits) - 1) : 255.0 / (219.0 * up);
    const double sc = full ? sy : 255.0 / (224.0 * up);
    const double iy = 1.0 / (sy * up), ic = 1.0 / (sc * up);   // the reciprocal scales at 8 bits: the shift makes the depth
    t.k.cy = yuv_ex_round(sy);
    t.k.cub = yuv_ex_round(2.0 * (1.0 - kb) * sc);
    t.k.cug = yuv_ex_round(-2.0 * kb * (1.0 - kb) / kg * sc);
    t.k.cvg = yuv_ex_round(-2.0 * kr * (1.0 - kr) / kg * sc);
    t.k.cvr = yuv_ex_round(2.0 * (1.0 - kr) * sc);
    t.k.ry = yuv_ex_round(kr * iy);
    t.k.gy = yuv_ex_round(kg * iy);
    t.k.by = yuv_ex_round(kb * iy);
    t.k.ru = yuv_ex_round(-kr / (2.0 * (1.0 - kb)) * ic);
    t.k.gu = yuv_ex_round(-kg / (2.0 * (1.0 - kb)) * ic);
    t.k.bu = yuv_ex_round(0.5 * ic);
    t.k.rv = yuv_ex_round(0.5 * ic);
    t.k.gv = yuv_ex_round(-kg / (2.0 * (1.0 - kr)) * ic);
    t.k.bv = yuv_ex_round(-kb / (2.0 * (1.0 - kr)) * ic);
    return t;
}

// clamp(s >> shift) to 0 .. 2^n - 1 with n + shift = 28 + log2n, as the clamp of s before the shift (yuv_shift_clamp's order and
// reason); `top` is 2^(28 + log2n) - 1
OCVAR_HD int yuv_ex_shift_clamp(int s, int top, int shift) { return (s < 0 ? 0 : (s > top ? top : s)) >> shift; }

// YUV to colour in yuv_core.h's three steps (yuv_channel is its own)
OCVAR_HD void yuv_ex_terms(const YuvCoefEx& k, int U, int V, bool rgb, int* t) {
    const int u = U - k.c_mid, v = V - k.c_mid;
    const int tb = yuv_mul(k.k.cub, u), tr = yuv_mul(k.k.cvr, v);
    t[0] = rgb ? tr : tb;
    t[1] = yuv_mul(k.k.cvg, v) + yuv_mul(k.k.cug, u);
    t[2] = rgb ? tb : tr;
}
OCVAR_HD int yuv_ex_y_term(const YuvCoefEx& k, int Y) { return yuv_mul(Y > k.y_off ? Y - k.y_off : 0, k.k.cy) + YUV_HALF; }

OCVAR_HD void yuv_ex_to_bgr(const YuvCoefEx& k, int Y, int U, int V, int* B, int* G, int* R) {
    int t[3];
    yuv_ex_terms(k, U, V, false, t);
    const int y = yuv_ex_y_term(k, Y);
    *B = yuv_channel(y, t[0]);
    *G = yuv_channel(y, t[1]);
    *R = yuv_channel(y, t[2]);
}

OCVAR_HD int yuv_ex_luma(const YuvCoefEx& k, int B, int G, int R) {
    const int half = 1 << (k.out_shift - 1);
    return yuv_ex_shift_clamp(yuv_mul(k.k.ry, R) + yuv_mul(k.k.gy, G) + yuv_mul(k.k.by, B) + half + k.out_y_off, (1 << 28) - 1, k.out_shift);
}

// U and V of the 2^log2n pixels (log2n 0, 1 or 2) whose channel sums are sB, sG, sR
OCVAR_HD void yuv_ex_chroma(const YuvCoefEx& k, int sB, int sG, int sR, int log2n, int* U, int* V) {
    const int shift = k.out_shift + log2n;
    const int bias = (1 << (shift - 1)) + (k.c_mid << shift), top = (1 << (28 + log2n)) - 1;
    *U = yuv_ex_shift_clamp(yuv_mul(k.k.ru, sR) + yuv_mul(k.k.gu, sG) + yuv_mul(k.k.bu, sB) + bias, top, shift);
    *V = yuv_ex_shift_clamp(yuv_mul(k.k.rv, sR) + yuv_mul(k.k.gv, sG) + yuv_mul(k.k.bv, sB) + bias, top, shift);
}

OCVAR_HD YuvCoefEx yuv_ex_coef_in_memory_order(const YuvCoefEx& k, bool rgb) {
    YuvCoefEx m = k;
    m.k = yuv_coef_in_memory_order(k.k, rgb);
    return m;
}

// One launch's arguments: YuvArgs with the wider table and the bytes of a sample (1, or 2: little-endian words).
struct YuvExArgs {
    uint8_t* y;
    uint8_t* c0;
    uint8_t* c1;
    long long y_pitch, c_pitch, yuv_frame_stride;
    uint8_t* pix;
    long long pix_row_stride, pix_frame_stride;
    int W, H, layout, format, sample_bytes;
    YuvCoefEx k;
};

// Where the samples of pixel (x, y) lie, from the frame's plane starts (fo: the frame's offset).
OCVAR_HD uint8_t* yuv_ex_y_at(const YuvExArgs& a, long long fo, int x, int y) {
    const int sub = yuv_ex_sub(a.layout);
    const long long in_row = sub == YUV_SUB_422 ? 2 * x + (a.layout == OCVAR_YUV_UYVY ? 1 : 0) : (long long)x * a.sample_bytes;
    return a.y + fo + (long long)y * a.y_pitch + in_row;
}
OCVAR_HD void yuv_ex_uv_at(const YuvExArgs& a, long long fo, int x, int y, uint8_t** pu, uint8_t** pv) {
    if (yuv_ex_semiplanar(a.layout)) {
        uint8_t* p = a.c0 + fo + (long long)(y >> 1) * a.c_pitch + (long long)(x & ~1) * a.sample_bytes;
        const bool vu = a.layout == OCVAR_YUV_NV21;
        *pu = p + (vu ? a.sample_bytes : 0);
        *pv = p + (vu ? 0 : a.sample_bytes);
    } else if (a.layout == OCVAR_YUV_I420) {
        const long long o = fo + (long long)(y >> 1) * a.c_pitch + (x >> 1);
        *pu = a.c0 + o;
        *pv = a.c1 + o;
    } else if (a.layout == OCVAR_YUV_I444) {
        const long long o = fo + (long long)y * a.c_pitch + x;
        *pu = a.c0 + o;
        *pv = a.c1 + o;
    } else {
        uint8_t* p = a.y + fo + (long long)y * a.y_pitch + 4 * (x >> 1) + (a.layout == OCVAR_YUV_UYVY ? 0 : 1);
        *pu = p;
        *pv = p + 2;
    }
}
// a sample at p (16-bit samples lie at even addresses: yuv_ex_check)
inline int yuv_ex_get(const YuvExArgs& a, const uint8_t* p) {
    return a.sample_bytes == 2 ? (int)(*reinterpret_cast<const uint16_t*>(p)) >> a.k.word_shift : (int)*p;
}
inline void yuv_ex_put(const YuvExArgs& a, uint8_t* p, int s) {
    if (a.sample_bytes == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)(s << a.k.word_shift);
    else *p = (uint8_t)s;
}

// The host reference of YUV to colour: frame f of the launch, sequentially.
inline void yuv_ex_to_frame(const YuvExArgs& a, int f) {
    const int bpp = format_bpp(a.format);
    const bool rgb = yuv_fmt_rgb(a.format);
    const long long fo = (long long)f * a.yuv_frame_stride;
    for (int y = 0; y < a.H; y++)
        for (int x = 0; x < a.W; x++) {
            uint8_t *pu, *pv;
            yuv_ex_uv_at(a, fo, x, y, &pu, &pv);
            int B, G, R;
            yuv_ex_to_bgr(a.k, yuv_ex_get(a, yuv_ex_y_at(a, fo, x, y)), yuv_ex_get(a, pu), yuv_ex_get(a, pv), &B, &G, &R);
            uint8_t* out = a.pix + (long long)f * a.pix_frame_stride + (long long)y * a.pix_row_stride + (long long)x * bpp;
            for (int c = 0; c < bpp; c++) out[c] = (uint8_t)yuv_pixel_byte(bpp, rgb, c, B, G, R);
        }
}

// The host reference of colour to YUV: frame f of the launch, sequentially.
inline void yuv_ex_from_frame(const YuvExArgs& a, int f) {
    const int bpp = format_bpp(a.format);
    const bool rgb = yuv_fmt_rgb(a.format);
    const long long fo = (long long)f * a.yuv_frame_stride;
    const int sub = yuv_ex_sub(a.layout);
    const int bw = sub == YUV_SUB_444 ? 1 : 2, bh = sub == YUV_SUB_420 ? 2 : 1;   // a chroma sample's block
    for (int y0 = 0; y0 < a.H; y0 += bh)
        for (int x0 = 0; x0 < a.W; x0 += bw) {
            int sB = 0, sG = 0, sR = 0;
            for (int dy = 0; dy < bh; dy++)
                for (int dx = 0; dx < bw; dx++) {
                    const uint8_t* p = a.pix + (long long)f * a.pix_frame_stride + (long long)(y0 + dy) * a.pix_row_stride + (long long)(x0 + dx) * bpp;
                    int B, G, R;
                    yuv_pixel_colour(bpp, rgb, p[0], bpp > 1 ? p[1] : 0, bpp > 1 ? p[2] : 0, &B, &G, &R);
                    yuv_ex_put(a, yuv_ex_y_at(a, fo, x0 + dx, y0 + dy), yuv_ex_luma(a.k, B, G, R));
                    sB += B;
                    sG += G;
                    sR += R;
                }
            int U, V;
            yuv_ex_chroma(a.k, sB, sG, sR, 2 - sub, &U, &V);   // (4, 2 or 1 pixels)
            uint8_t *pu, *pv;
            yuv_ex_uv_at(a, fo, x0, y0, &pu, &pv);
            yuv_ex_put(a, pu, U);
            yuv_ex_put(a, pv, V);
        }
}

// ---- what the entry points refuse ----------------------------------------------------------------------------------------------------

// Why a call is refused, in the order the faults are looked for (0: it is not).
enum YuvExBad {
    YUV_EX_OK = 0,
    YUV_EX_NO_FRAMES,     // no descriptor or no frames
    YUV_EX_UNKNOWN,       // an unknown layout, matrix, range, depth or format
    YUV_EX_DEPTH_LAYOUT,  // more than 8 bits with a layout other than NV12
    YUV_EX_NO_PLANE,      // a plane the layout uses is NULL
    YUV_EX_SIDE,          // sides outside 1 .. the limit, or n_frames < 1
    YUV_EX_ROW_STRIDE,    // a row stride below the format's bytes per pixel times width
    YUV_EX_SPAN,          // the rows of a plane or of a frame span more than 2^31 - 1 bytes
    YUV_EX_ODD_SIDE,      // an odd width or height with a layout that subsamples along it
    YUV_EX_ODD_WORDS,     // 16-bit samples at an odd address, pitch or frame stride
    YUV_EX_PITCH,         // a pitch below the plane's bytes per row
    YUV_EX_OVERLAP,       // the byte ranges of a plane and of the frames intersect
};

// The planes of a descriptor as blocks of bytes (a packed row has two bytes per pixel, a row of 16-bit samples two per sample) ->
// their number.  Sides are taken as they are: the caller has checked them.
inline int yuv_ex_planes(const OcvarYuvFramesEx& d, int width, int height, int n_frames, FrameBlock* planes) {
    const int sub = yuv_ex_sub(d.layout), sb = d.bits > 8 ? 2 : 1;
    const uint8_t *y = (const uint8_t*)d.y, *c0 = (const uint8_t*)d.c0, *c1 = (const uint8_t*)d.c1;
    int n = 0;
    planes[n++] = FrameBlock{y, sub == YUV_SUB_422 ? 2 * width : width * sb, height, 1, d.y_pitch, d.frame_stride, n_frames};
    if (yuv_ex_semiplanar(d.layout)) planes[n++] = FrameBlock{c0, width * sb, height / 2, 1, d.c_pitch, d.frame_stride, n_frames};
    if (d.layout == OCVAR_YUV_I420 || d.layout == OCVAR_YUV_I444) {
        const int cw = sub == YUV_SUB_444 ? width : width / 2, ch = sub == YUV_SUB_444 ? height : height / 2;
        planes[n++] = FrameBlock{c0, cw, ch, 1, d.c_pitch, d.frame_stride, n_frames};
        planes[n++] = FrameBlock{c1, cw, ch, 1, d.c_pitch, d.frame_stride, n_frames};
    }
    return n;
}

inline int yuv_ex_frames_bad(int bad) {
    return bad == FRAMES_OK ? YUV_EX_OK : (bad == FRAMES_FORMAT ? YUV_EX_UNKNOWN : (bad == FRAMES_ROW_STRIDE ? YUV_EX_ROW_STRIDE :
           (bad == FRAMES_SPAN ? YUV_EX_SPAN : YUV_EX_SIDE)));
}

// d describes one side, the block at pix the other; max_w x max_h: the largest frame (the context's size).
inline int yuv_ex_check(const OcvarYuvFramesEx* d, const uint8_t* pix, int row_stride, size_t frame_stride, int width, int height, int n_frames,
                        int format, int max_w, int max_h) {
    if (!d || !pix) return YUV_EX_NO_FRAMES;
    if (!yuv_ex_layout_ok(d->layout) || !yuv_ex_matrix_ok(d->matrix) || !yuv_ex_range_ok(d->range) || !yuv_ex_bits_ok(d->bits)) return YUV_EX_UNKNOWN;
    if (d->bits > 8 && d->layout != OCVAR_YUV_NV12) return YUV_EX_DEPTH_LAYOUT;
    const int sub = yuv_ex_sub(d->layout);
    const bool two = d->layout != OCVAR_YUV_YUYV && d->layout != OCVAR_YUV_UYVY, three = d->layout == OCVAR_YUV_I420 || d->layout == OCVAR_YUV_I444;
    if (!d->y || (two && !d->c0) || (three && !d->c1)) return YUV_EX_NO_PLANE;
    const FrameBlock frames{pix, width, height, format_bpp(format), row_stride, frame_stride, n_frames};
    if (int bad = frames_check(frames, max_w, max_h)) return yuv_ex_frames_bad(bad);
    if ((sub != YUV_SUB_444 && (width & 1)) || (sub == YUV_SUB_420 && (height & 1))) return YUV_EX_ODD_SIDE;
    if (d->bits > 8 && (((uintptr_t)d->y | (uintptr_t)d->c0 | (uintptr_t)d->y_pitch | (uintptr_t)d->c_pitch | (uintptr_t)d->frame_stride) & 1))
        return YUV_EX_ODD_WORDS;
    FrameBlock planes[3];
    const int n_planes = yuv_ex_planes(*d, width, height, n_frames, planes);
    for (int i = 0; i < n_planes; i++) {
        if (planes[i].row_stride < planes[i].width) return YUV_EX_PITCH;
        if (int bad = frames_check(planes[i], 2 * max_w, max_h)) return yuv_ex_frames_bad(bad);
        if (frames_intersect(planes[i], frames)) return YUV_EX_OVERLAP;
    }
    return YUV_EX_OK;
}

inline YuvExArgs yuv_ex_args(const OcvarYuvFramesEx& d, size_t f0, const uint8_t* pix, int row_stride, size_t frame_stride, int width, int height,
                             int format) {
    const size_t yo = f0 * d.frame_stride;
    uint8_t *y = (uint8_t*)d.y, *c0 = (uint8_t*)d.c0, *c1 = (uint8_t*)d.c1;
    return YuvExArgs{y + yo, c0 ? c0 + yo : nullptr, c1 ? c1 + yo : nullptr, (long long)d.y_pitch, (long long)d.c_pitch, (long long)d.frame_stride,
                     const_cast<uint8_t*>(pix) + f0 * frame_stride, (long long)row_stride, (long long)frame_stride, width, height, d.layout, format,
                     d.bits > 8 ? 2 : 1, yuv_coef_ex(d.matrix, d.range, d.bits)};
}

}  // namespace ocvar

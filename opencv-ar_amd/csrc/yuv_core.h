// yuv_core.h -- 8-bit limited-range YUV frames (NV12, I420, YUYV, UYVY) to and from the interleaved frame formats, on frames
// that stay in device memory (opt-in: ocvar_hip_yuv_to_frames / ocvar_hip_frames_to_yuv).  What a video decoder delivers becomes
// what detection, overlays, patches, undistortion and flow take, and a rendered frame becomes what an encoder takes.  The calls
// stand for OpenCV's cvtColor with COLOR_YUV2BGR_NV12 / _I420 / _YUY2 / _UYVY and COLOR_BGR2YUV_I420 (and their RGB, four-channel
// and grey relatives).  No counterpart in the reference, which converts nothing.
//
// Everything is integer arithmetic in a 20-bit fixed point (YUV_SHIFT), with a floor shift and a clamp to 0 .. 255:
//   YUV to colour   u = U - 128, v = V - 128, y = max(Y - 16, 0) * CY
//                     R = clamp((y + 2^19 + CVR v) >> 20)
//                     G = clamp((y + 2^19 + CVG v + CUG u) >> 20)
//                     B = clamp((y + 2^19 + CUB u) >> 20)
//                   (the sums can be negative: >> on a signed int is the floor shift)
//   colour to Y     Y = clamp((RY R + GY G + BY B + 2^19 + (16 << 20)) >> 20), per pixel
//   colour to U, V  per chroma sample, from the channel sums sR sG sB over the n = 2^log2n pixels that share it (4 for 4:2:0, 2 for
//                   4:2:2):
//                     U = clamp((RU sR + GU sG + BU sB + (2^19 << log2n) + (128 << (20 + log2n))) >> (20 + log2n))
//                     V = the same with RV GV BV
//                   (these sums are never negative; for 8-bit input Y lies in 16 .. 235 and U, V in 16 .. 240 before the clamp)
// No sum leaves the range of an int: the largest is below 2^30 (tests/test_yuv_cpu.py runs all 2^24 inputs of each formula).
//
// The coefficients are a table (YuvCoef) that travels by value in the launch arguments; the kernels do not know which they hold.
//   OCVAR_YUV_BT601  the constants of OpenCV's cvtColor YUV family (ITUR_BT_601_*), written down from memory of OpenCV: no OpenCV
//                    exists where this library is built and tested, so parity with an OpenCV build is unpinned, as it is for
//                    undistort_core.h and flow_core.h.  The values below are the definition.
//   OCVAR_YUV_BT709  round(x * 2^20) of the BT.709 matrix, Kr = 0.2126, Kb = 0.0722, with the scales 255/219 and 255/224.
// Both are limited range (Y 16 .. 235, U V 16 .. 240).  Full range is not offered.
//
// Layouts.  NV12: a Y plane, then one plane of interleaved U V at half resolution.  I420: Y, U and V planes.  YUYV: one plane of
// Y0 U Y1 V.  UYVY: one plane of U Y0 V Y1.  In 4:2:0 chroma sample (i, j) belongs to pixels (2i .. 2i+1, 2j .. 2j+1), in 4:2:2 to
// pixels 2i .. 2i+1 of one row.  YUV to colour uses the sample as it is (nearest, no interpolation, as OpenCV does).  Widths are
// even; heights are even in 4:2:0.
//
// The interleaved side is any OCVAR_FMT_*.  As a target BGRA and RGBA get byte 3 = 255, and GRAY gets the library's grey of the
// converted colour, (1868 B + 9617 G + 4899 R + 8192) >> 14: detection on it is detection on the converted BGR frame.  As a source
// byte 3 is ignored and GRAY reads as B = G = R = g.
//
// The host build (tests/emul/yuv_emul.cpp) gives the bytes of the kernels (yuv.hip).  yuv_to_frame and frame_to_yuv are that host
// reference, sequential, pixel by pixel.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "patch_core.h"

namespace ocvar {

constexpr int YUV_SHIFT = 20;
constexpr int YUV_HALF = 1 << (YUV_SHIFT - 1);

struct YuvCoef {
    int cy, cub, cug, cvg, cvr;   // YUV to colour
    int ry, gy, by;               // colour to Y
    int ru, gu, bu;               // colour to U
    int rv, gv, bv;               // colour to V
};

constexpr YuvCoef YUV_COEF_BT601 = {1220542, 2116026, -409993, -852492, 1673527, 269484, 528482, 102760,
                                    -155188, -305135, 460324, 460324, -385875, -74448};
constexpr YuvCoef YUV_COEF_BT709 = {1220945, 2215014, -223607, -558796, 1879825, 191455, 644067, 65019,
                                    -105533, -355018, 460551, 460551, -418321, -42230};

inline bool yuv_matrix_ok(int matrix) { return matrix == OCVAR_YUV_BT601 || matrix == OCVAR_YUV_BT709; }
inline YuvCoef yuv_coef(int matrix) { return matrix == OCVAR_YUV_BT709 ? YUV_COEF_BT709 : YUV_COEF_BT601; }
OCVAR_HD bool yuv_layout_ok(int layout) { return layout >= OCVAR_YUV_NV12 && layout <= OCVAR_YUV_UYVY; }
OCVAR_HD bool yuv_is_420(int layout) { return layout == OCVAR_YUV_NV12 || layout == OCVAR_YUV_I420; }

// clamp(s >> shift) to 0 .. 255, computed as the clamp of s to 0 .. 2^(8 + shift) - 1 before the shift -- the same number for every
// int s (s < 0 floors below 0; s >= 2^(8 + shift) floors to 256 or more).  The order matters to the compiler only: from "shift,
// then clamp" of two neighbouring bytes it builds gfx950's v_ashr_pk_u8_i32 and reads its result as a zero-extended 16-bit value,
// while the instruction left the destination's upper half as it was on the MI355X this was first run on (DESIGN.md, section YUV).
OCVAR_HD int yuv_shift_clamp(int s, int shift) {
    const int top = (256 << shift) - 1;
    return (s < 0 ? 0 : (s > top ? top : s)) >> shift;
}

// a * b for |a|, |b| < 2^23 (every coefficient is; the other factor is a byte, a byte - 128 or a sum of four bytes): the 24-bit
// multiplier on the device, four times the rate of the 32-bit one
OCVAR_HD int yuv_mul(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// YUV to colour in three steps, so that a kernel computes the chroma terms once for the pixels that share a sample.  t[0 .. 2] are
// the terms of the channels in memory order: B G R, or R G B when rgb.
OCVAR_HD void yuv_terms(const YuvCoef& k, int U, int V, bool rgb, int* t) {
    const int u = U - 128, v = V - 128;
    const int tb = yuv_mul(k.cub, u), tr = yuv_mul(k.cvr, v);
    t[0] = rgb ? tr : tb;
    t[1] = yuv_mul(k.cvg, v) + yuv_mul(k.cug, u);
    t[2] = rgb ? tb : tr;
}
OCVAR_HD int yuv_y_term(const YuvCoef& k, int Y) { return yuv_mul(Y > 16 ? Y - 16 : 0, k.cy) + YUV_HALF; }
OCVAR_HD int yuv_channel(int y_term, int t) { return yuv_shift_clamp(y_term + t, YUV_SHIFT); }

OCVAR_HD void yuv_to_bgr(const YuvCoef& k, int Y, int U, int V, int* B, int* G, int* R) {
    int t[3];
    yuv_terms(k, U, V, false, t);
    const int y = yuv_y_term(k, Y);
    *B = yuv_channel(y, t[0]);
    *G = yuv_channel(y, t[1]);
    *R = yuv_channel(y, t[2]);
}

OCVAR_HD int yuv_luma(const YuvCoef& k, int B, int G, int R) {
    return yuv_shift_clamp(yuv_mul(k.ry, R) + yuv_mul(k.gy, G) + yuv_mul(k.by, B) + YUV_HALF + (16 << YUV_SHIFT), YUV_SHIFT);
}

// U and V of the 2^log2n pixels whose channel sums are sB, sG, sR
OCVAR_HD void yuv_chroma(const YuvCoef& k, int sB, int sG, int sR, int log2n, int* U, int* V) {
    const int bias = (YUV_HALF << log2n) + (128 << (YUV_SHIFT + log2n));
    *U = yuv_shift_clamp(yuv_mul(k.ru, sR) + yuv_mul(k.gu, sG) + yuv_mul(k.bu, sB) + bias, YUV_SHIFT + log2n);
    *V = yuv_shift_clamp(yuv_mul(k.rv, sR) + yuv_mul(k.gv, sG) + yuv_mul(k.bv, sB) + bias, YUV_SHIFT + log2n);
}

// The table with the roles of R and B exchanged: with it the bytes 0 1 2 of an RGB pixel serve as B G R in yuv_luma and yuv_chroma.
OCVAR_HD YuvCoef yuv_coef_in_memory_order(const YuvCoef& k, bool rgb) {
    YuvCoef m = k;
    if (rgb) {
        m.ry = k.by; m.by = k.ry;
        m.ru = k.bu; m.bu = k.ru;
        m.rv = k.bv; m.bv = k.rv;
    }
    return m;
}

OCVAR_HD int yuv_grey(int B, int G, int R) { return (1868 * B + 9617 * G + 4899 * R + 8192) >> 14; }
OCVAR_HD bool yuv_fmt_rgb(int fmt) { return fmt == OCVAR_FMT_RGB || fmt == OCVAR_FMT_RGBA; }

// Byte c (0 .. bpp - 1) of a pixel of the colour (B, G, R) in a format of bpp bytes, rgb: the channels reversed.
OCVAR_HD int yuv_pixel_byte(int bpp, bool rgb, int c, int B, int G, int R) {
    if (bpp == 1) return yuv_grey(B, G, R);
    return c == 0 ? (rgb ? R : B) : (c == 1 ? G : (c == 2 ? (rgb ? B : R) : 255));
}

// The colour of a pixel whose first three bytes are p0 p1 p2 (bpp 1: p0 only).
OCVAR_HD void yuv_pixel_colour(int bpp, bool rgb, int p0, int p1, int p2, int* B, int* G, int* R) {
    if (bpp == 1) {
        *B = *G = *R = p0;
    } else {
        *B = rgb ? p2 : p0;
        *G = p1;
        *R = rgb ? p0 : p2;
    }
}

// One launch's arguments, all pointers in device memory: frame f's planes start yuv_frame_stride bytes after frame f - 1's, rows
// y_pitch (Y or the packed plane) and c_pitch (chroma planes) bytes apart; its pixels start pix_frame_stride after frame f - 1's,
// rows pix_row_stride apart.  c0: NV12 the U V plane, I420 the U plane; c1: I420 the V plane.  Either side is the source.
struct YuvArgs {
    uint8_t* y;
    uint8_t* c0;
    uint8_t* c1;
    long long y_pitch, c_pitch, yuv_frame_stride;
    uint8_t* pix;
    long long pix_row_stride, pix_frame_stride;
    int W, H, layout, format;
    YuvCoef k;
};

// Where the samples of pixel (x, y) lie: byte offsets from the frame's plane starts.
OCVAR_HD long long yuv_y_off(const YuvArgs& a, int x, int y) {
    return (long long)y * a.y_pitch + (yuv_is_420(a.layout) ? x : 2 * x + (a.layout == OCVAR_YUV_UYVY ? 1 : 0));
}
// the U sample of pixel (x, y) is at *base + off, the V sample at *base_v + off_v
OCVAR_HD void yuv_uv_at(const YuvArgs& a, long long fo, int x, int y, uint8_t** pu, uint8_t** pv) {
    if (a.layout == OCVAR_YUV_NV12) {
        uint8_t* p = a.c0 + fo + (long long)(y >> 1) * a.c_pitch + (x & ~1);
        *pu = p;
        *pv = p + 1;
    } else if (a.layout == OCVAR_YUV_I420) {
        const long long o = fo + (long long)(y >> 1) * a.c_pitch + (x >> 1);
        *pu = a.c0 + o;
        *pv = a.c1 + o;
    } else {
        uint8_t* p = a.y + fo + (long long)y * a.y_pitch + 4 * (x >> 1) + (a.layout == OCVAR_YUV_UYVY ? 0 : 1);
        *pu = p;
        *pv = p + 2;
    }
}

// The host reference of YUV to colour: frame f of the launch, sequentially.
inline void yuv_to_frame(const YuvArgs& a, int f) {
    const int bpp = format_bpp(a.format);
    const bool rgb = yuv_fmt_rgb(a.format);
    const long long fo = (long long)f * a.yuv_frame_stride;
    for (int y = 0; y < a.H; y++)
        for (int x = 0; x < a.W; x++) {
            uint8_t *pu, *pv;
            yuv_uv_at(a, fo, x, y, &pu, &pv);
            int B, G, R;
            yuv_to_bgr(a.k, a.y[fo + yuv_y_off(a, x, y)], *pu, *pv, &B, &G, &R);
            uint8_t* out = a.pix + (long long)f * a.pix_frame_stride + (long long)y * a.pix_row_stride + (long long)x * bpp;
            for (int c = 0; c < bpp; c++) out[c] = (uint8_t)yuv_pixel_byte(bpp, rgb, c, B, G, R);
        }
}

// The host reference of colour to YUV: frame f of the launch, sequentially.
inline void frame_to_yuv(const YuvArgs& a, int f) {
    const int bpp = format_bpp(a.format);
    const bool rgb = yuv_fmt_rgb(a.format);
    const long long fo = (long long)f * a.yuv_frame_stride;
    const int bh = yuv_is_420(a.layout) ? 2 : 1;   // rows of a chroma sample's block
    for (int y0 = 0; y0 < a.H; y0 += bh)
        for (int x0 = 0; x0 < a.W; x0 += 2) {
            int sB = 0, sG = 0, sR = 0;
            for (int dy = 0; dy < bh; dy++)
                for (int dx = 0; dx < 2; dx++) {
                    const uint8_t* p = a.pix + (long long)f * a.pix_frame_stride + (long long)(y0 + dy) * a.pix_row_stride + (long long)(x0 + dx) * bpp;
                    int B, G, R;
                    yuv_pixel_colour(bpp, rgb, p[0], bpp > 1 ? p[1] : 0, bpp > 1 ? p[2] : 0, &B, &G, &R);
                    a.y[fo + yuv_y_off(a, x0 + dx, y0 + dy)] = (uint8_t)yuv_luma(a.k, B, G, R);
                    sB += B;
                    sG += G;
                    sR += R;
                }
            int U, V;
            yuv_chroma(a.k, sB, sG, sR, bh, &U, &V);   // (2^bh pixels: 4 in 4:2:0, 2 in 4:2:2)
            uint8_t *pu, *pv;
            yuv_uv_at(a, fo, x0, y0, &pu, &pv);
            *pu = (uint8_t)U;
            *pv = (uint8_t)V;
        }
}

}  // namespace ocvar

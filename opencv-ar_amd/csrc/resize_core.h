// resize_core.h -- device-resident frames brought to another size, and marker records carried between the two sizes (opt-in:
// ocvar_hip_resize / ocvar_hip_scale_records).  A 3840 x 2160 stream is detected at 1920 x 1080 by a context sized for that, and
// the records found there are drawn on the large frames.  The frame call stands for OpenCV's resize(src, dst, dsize, 0, 0,
// interpolation) on 8-bit images with every byte of a pixel treated alike, byte 3 of a four-channel pixel included: a GRAY frame
// resizes like any one-channel image.  The reference has cvarCameraScale for the camera and nothing for frames or records.
//
// No OpenCV exists where this library is built and tested: the rules are written down from memory of the 2.4 / 3.x source, so
// parity with an OpenCV build is unpinned, as it is for undistort_core.h, flow_core.h and yuv_core.h.  This header is the
// definition; the tests pin it.
//
// Per axis, s the source extent and d the destination extent: scale = 1.0 / ((double)d / (double)s) -- two roundings, as OpenCV
// computes it (resize_scale).
//   NEAREST  sx = min((int)floor(x * scale_x), sw - 1), likewise in y.
//   LINEAR   fx = (float)((x + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx; sx < 0: sx = 0, fx = 0; sx >= sw - 1: sx = sw - 1,
//            fx = 0; the second tap is min(sx + 1, sw - 1).  a0 = rn_even((1.f - fx) * 2048), a1 = rn_even(fx * 2048), each rounded
//            on its own (shorts; they need not sum to 2048); sy, b0, b1 alike.  In int32
//              r0 = S[sy][sx] a0 + S[sy][sx1] a1, r1 the same on row sy1,
//              D = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.
//            A LINEAR call whose two scales are both exactly 2 is the AREA result (OpenCV switches it, and so does this).
//   AREA     for dw <= sw and dh <= sh only, sw <= 16 dw and sh <= 16 dh (OCVAR_MAX_RESIZE_RATIO).  iscale = rn_even(scale) per
//            axis; when |scale - iscale| < DBL_EPSILON on both axes the pixel is the int32 sum of its iscale_x x iscale_y block,
//            stored as (sum + 2) >> 2 for the 2 x 2 block and as rn_even_sat_u8((float)sum * (float)(1.0 / area)) for every other.
//            Otherwise the table of computeResizeAreaTab per axis, for destination index i:
//              f1 = i * scale, f2 = f1 + scale, cell = min(scale, s - f1), s1 = ceil(f1), s2 = min(floor(f2), s - 1), s1 = min(s1, s2);
//              a leading tap at s1 - 1 of weight (float)((s1 - f1) / cell) when s1 - f1 > 1e-3; full taps s1 .. s2 - 1 of weight
//              (float)(1.0 / cell); a trailing tap at s2 of weight (float)(min(min(f2 - s2, 1.0), cell) / cell) when f2 - s2 > 1e-3.
//            A byte is accumulated in float in this order and no other: for each source row in table order, row = the sum over
//            the x taps in table order of (float)S * alpha; then acc += beta * row; the byte is rn_even_sat_u8(acc).
//   records  a source coordinate p becomes (p + 0.5) * ((double)d / (double)s) - 0.5, in double per axis (the pixel-centre rule of
//            the linear map), rounded to float32, a NaN stored as 0x7FC00000 (undistort_core.h: undistort_stored).  On an axis
//            whose two extents are equal the coordinate is copied as it is: with equal sizes the square is copied unchanged.
//            Every other field of the record is copied; with OCVAR_SCALE_POSE glMatrix is solved from the new square
//            (square_to_glmatrix with the camera of the call -- that of the destination size -- and the record's aspectRatio).
//            Slot k of a frame is written when k < min(count, slots); the other slots are not touched.
//
// All arithmetic is integer, IEEE float or IEEE double without contraction (-ffp-contract=off on both sides): the host build
// (tests/emul/resize_emul.cpp) gives the bytes of the kernels (resize.hip).  resize_frame and resize_records are that host
// reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "patch_core.h"
#include "pose_core.h"
#include "tail_core.h"
#include "undistort_core.h"
#include <float.h>
#include <math.h>

namespace ocvar {

constexpr int RESIZE_MAX_SIDE = 32767;
constexpr int RESIZE_MAX_RATIO = OCVAR_MAX_RESIZE_RATIO;
constexpr int RESIZE_FLAGS = OCVAR_SCALE_POSE;

// what a call comes down to: one of four per-pixel rules
enum { RESIZE_KIND_NEAREST = 0, RESIZE_KIND_LINEAR = 1, RESIZE_KIND_BOX = 2, RESIZE_KIND_TABLE = 3 };

struct ResizePlan {
    int kind;
    int kx, ky;                 // BOX: the block
    float inv_area;             // BOX: (float)(1.0 / (kx ky))
    double scale_x, scale_y;
};

inline double resize_scale(int s, int d) { return 1.0 / ((double)d / (double)s); }

inline bool resize_interp_ok(int interp) { return interp >= OCVAR_RESIZE_NEAREST && interp <= OCVAR_RESIZE_AREA; }
// AREA only shrinks, by at most RESIZE_MAX_RATIO per axis
inline bool resize_area_ok(int sw, int sh, int dw, int dh) {
    return dw <= sw && dh <= sh && (long long)sw <= (long long)RESIZE_MAX_RATIO * dw && (long long)sh <= (long long)RESIZE_MAX_RATIO * dh;
}

// The rule of a call (sides 1 .. RESIZE_MAX_SIDE, interp known, resize_area_ok for AREA).
inline ResizePlan resize_plan(int sw, int sh, int dw, int dh, int interp) {
    ResizePlan p;
    p.scale_x = resize_scale(sw, dw);
    p.scale_y = resize_scale(sh, dh);
    p.kx = p.ky = 1;
    p.inv_area = 1.0f;
    if (interp == OCVAR_RESIZE_LINEAR && p.scale_x == 2.0 && p.scale_y == 2.0) interp = OCVAR_RESIZE_AREA;
    if (interp == OCVAR_RESIZE_NEAREST) {
        p.kind = RESIZE_KIND_NEAREST;
    } else if (interp == OCVAR_RESIZE_LINEAR) {
        p.kind = RESIZE_KIND_LINEAR;
    } else {
        const int ix = (int)rint(p.scale_x), iy = (int)rint(p.scale_y);
        // (an integer scale is the ratio of the extents: the products only repeat that for the addresses' sake)
        const bool whole = fabs(p.scale_x - ix) < DBL_EPSILON && fabs(p.scale_y - iy) < DBL_EPSILON && (long long)ix * dw == sw && (long long)iy * dh == sh;
        p.kind = whole ? RESIZE_KIND_BOX : RESIZE_KIND_TABLE;
        if (whole) {
            p.kx = ix;
            p.ky = iy;
            p.inv_area = (float)(1.0 / (double)(ix * iy));
        }
    }
    return p;
}

OCVAR_HD int resize_rn_even_sat_u8(float v) {
    const int r = (int)rintf(v);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

OCVAR_HD int resize_nearest_index(int x, double scale, int s) {
    const int sx = (int)floor(x * scale);
    return sx < s - 1 ? sx : s - 1;
}

// the two taps of destination index x of an axis and their 11-bit weights
struct ResizeLinearTap {
    int s0, s1, a0, a1;
};
OCVAR_HD ResizeLinearTap resize_linear_tap(int x, double scale, int s) {
    float fx = (float)((x + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) {
        sx = 0;
        fx = 0.0f;
    }
    if (sx >= s - 1) {
        sx = s - 1;
        fx = 0.0f;
    }
    ResizeLinearTap t;
    t.s0 = sx;
    t.s1 = sx + 1 < s - 1 ? sx + 1 : s - 1;
    t.a0 = (int)(short)rintf((1.0f - fx) * 2048.0f);
    t.a1 = (int)(short)rintf(fx * 2048.0f);
    return t;
}
// from the four bytes of a channel, p[row][column]
OCVAR_HD int resize_linear_value(int p00, int p01, int p10, int p11, const ResizeLinearTap& tx, const ResizeLinearTap& ty) {
    const int r0 = p00 * tx.a0 + p01 * tx.a1, r1 = p10 * tx.a0 + p11 * tx.a1;
    return (((ty.a0 * (r0 >> 4)) >> 16) + ((ty.a1 * (r1 >> 4)) >> 16) + 2) >> 2;
}

OCVAR_HD int resize_box_value(int sum, int kx, int ky, float inv_area) {
    return (kx == 2 && ky == 2) ? (sum + 2) >> 2 : resize_rn_even_sat_u8((float)sum * inv_area);
}

// The table's entries of destination index i of an axis: n taps at first, first + 1, ..., the first of weight lead when has_lead,
// the last of weight trail when has_trail, the others of weight full.
struct ResizeAreaSpan {
    int first, n;
    bool has_lead, has_trail;
    float lead, full, trail;
};
OCVAR_HD ResizeAreaSpan resize_area_span(int i, double scale, int s) {
    const double f1 = i * scale, f2 = f1 + scale;
    const double rest = s - f1, cell = scale < rest ? scale : rest;
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = s2 < s - 1 ? s2 : s - 1;
    s1 = s1 < s2 ? s1 : s2;
    ResizeAreaSpan t;
    t.has_lead = s1 - f1 > 1e-3;
    t.has_trail = f2 - s2 > 1e-3;
    t.lead = (float)((s1 - f1) / cell);
    t.full = (float)(1.0 / cell);
    const double over = f2 - s2, m = over < 1.0 ? over : 1.0;
    t.trail = (float)((m < cell ? m : cell) / cell);
    t.first = s1 - (t.has_lead ? 1 : 0);
    t.n = (t.has_lead ? 1 : 0) + (s2 - s1) + (t.has_trail ? 1 : 0);
    return t;
}
OCVAR_HD float resize_area_weight(const ResizeAreaSpan& t, int k) {
    return (t.has_lead && k == 0) ? t.lead : ((t.has_trail && k == t.n - 1) ? t.trail : t.full);
}

// One launch's arguments, all pointers in device memory: frame f's pixels start *_frame_stride bytes after frame f - 1's, rows
// *_row_stride apart; source and destination do not overlap.
struct ResizeArgs {
    const uint8_t* src;
    uint8_t* dst;
    int sw, sh, dw, dh;
    long long src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride;
    ResizePlan p;
};

// The bpp bytes of destination pixel (x, y) of a frame whose source pixels begin at src.
OCVAR_HD void resize_pixel(const ResizeArgs& a, const uint8_t* src, int bpp, int x, int y, int* out) {
    const auto at = [=](int ix, int iy, int c) -> int { return src[(long long)iy * a.src_row_stride + (long long)ix * bpp + c]; };
    if (a.p.kind == RESIZE_KIND_NEAREST) {
        const int sx = resize_nearest_index(x, a.p.scale_x, a.sw), sy = resize_nearest_index(y, a.p.scale_y, a.sh);
        for (int c = 0; c < bpp; c++) out[c] = at(sx, sy, c);
    } else if (a.p.kind == RESIZE_KIND_LINEAR) {
        const ResizeLinearTap tx = resize_linear_tap(x, a.p.scale_x, a.sw), ty = resize_linear_tap(y, a.p.scale_y, a.sh);
        for (int c = 0; c < bpp; c++) out[c] = resize_linear_value(at(tx.s0, ty.s0, c), at(tx.s1, ty.s0, c), at(tx.s0, ty.s1, c), at(tx.s1, ty.s1, c), tx, ty);
    } else if (a.p.kind == RESIZE_KIND_BOX) {
        for (int c = 0; c < bpp; c++) {
            int sum = 0;
            for (int r = 0; r < a.p.ky; r++)
                for (int k = 0; k < a.p.kx; k++) sum += at(x * a.p.kx + k, y * a.p.ky + r, c);
            out[c] = resize_box_value(sum, a.p.kx, a.p.ky, a.p.inv_area);
        }
    } else {
        const ResizeAreaSpan tx = resize_area_span(x, a.p.scale_x, a.sw), ty = resize_area_span(y, a.p.scale_y, a.sh);
        for (int c = 0; c < bpp; c++) {
            float acc = 0.0f;
            for (int r = 0; r < ty.n; r++) {
                float row = 0.0f;
                for (int k = 0; k < tx.n; k++) row += (float)at(tx.first + k, ty.first + r, c) * resize_area_weight(tx, k);
                acc += resize_area_weight(ty, r) * row;
            }
            out[c] = resize_rn_even_sat_u8(acc);
        }
    }
}

// The host reference of the frame call: frame f of the launch in format fmt, sequentially.
inline void resize_frame(const ResizeArgs& a, int fmt, int f) {
    const int bpp = format_bpp(fmt);
    const uint8_t* src = a.src + (long long)f * a.src_frame_stride;
    uint8_t* dst = a.dst + (long long)f * a.dst_frame_stride;
    for (int y = 0; y < a.dh; y++)
        for (int x = 0; x < a.dw; x++) {
            int px[4];
            resize_pixel(a, src, bpp, x, y, px);
            for (int c = 0; c < bpp; c++) dst[(long long)y * a.dst_row_stride + (long long)x * bpp + c] = (uint8_t)px[c];
        }
}

// The record map on one coordinate of an axis with extents s -> d, and on one square (8 floats; out may be sq).
OCVAR_HD float resize_coord(float p, int s, int d) {
    if (s == d) return p;
    return undistort_stored(((double)p + 0.5) * ((double)d / (double)s) - 0.5);
}
OCVAR_HD void resize_square(const float* sq, int sw, int sh, int dw, int dh, float* out) {
    for (int k = 0; k < 4; k++) {
        out[2 * k] = resize_coord(sq[2 * k], sw, dw);
        out[2 * k + 1] = resize_coord(sq[2 * k + 1], sh, dh);
    }
}

// One record as the call leaves it.
OCVAR_HD void resize_record(MarkerRec& r, int sw, int sh, int dw, int dh, int flags, const CameraRec& cam) {
    resize_square(r.square, sw, sh, dw, dh, r.square);
    if (flags & OCVAR_SCALE_POSE) {
        double gl[16];
        square_to_glmatrix(r.square, cam, r.aspectRatio, gl);
        for (int q = 0; q < 16; q++) r.glMatrix[q] = gl[q];
    }
}

// The host reference of the record call: slots k < min(count, slots) of one frame from in to out (which may be the same array).
// Returns the number of slots written.
inline int resize_records(const MarkerRec* in, int count, int slots, int sw, int sh, int dw, int dh, int flags, const CameraRec& cam,
                          MarkerRec* out) {
    const int n = count < slots ? count : slots;
    for (int k = 0; k < n; k++) {
        MarkerRec r = in[k];
        resize_record(r, sw, sh, dw, dh, flags, cam);
        out[k] = r;
    }
    return n < 0 ? 0 : n;
}

}  // namespace ocvar

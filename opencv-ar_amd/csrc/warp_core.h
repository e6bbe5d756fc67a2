// warp_core.h -- device-resident frames warped by one projective map per frame, the marker records carried along, and the map that
// shows a board's plane from straight above (opt-in: ocvar_hip_warp / ocvar_hip_warp_records / ocvar_hip_board_plane_maps).  The
// reference's public cvarInvertPerspective(input, output, src, dst) (opencvar.cpp:510-516: cvGetPerspectiveTransform +
// cvWarpPerspective) for any output size and any four points, with the sampler decode_core.h already has (invert_map, warp_fixed32,
// warp_sample_fixed, warp_sample_px) and nothing beyond it but the second interpolation and the second border.
//
//   map      nine doubles per frame, m[0..8] row by row.  By default the FORWARD map, source pixels -> destination pixels, as OpenCV's
//            warpPerspective takes it; it is inverted in double by invert_map's formula (the adjugate times 1 / det, the same
//            expressions in the same order).  With OCVAR_WARP_INVERSE_MAP the nine doubles already map destination -> source and are
//            used as they are.  A frame is SKIPPED when any of the nine is not finite, or when the forward map's determinant is 0 or
//            an entry of its inverse is not finite: status 0, none of its destination bytes touched.  Every other frame: status 1.
//   pixel    M the destination -> source map.  OCVAR_WARP_LINEAR: byte c of destination pixel (x, y) is warp_sample_px's arithmetic,
//            unchanged: X0 = M[0] * 0 + M[1] * y + M[2], Y0, W0 alike, W = W0 + M[6] * x, W = W ? 32. / W : 0,
//            X = warp_fixed32((X0 + M[0] * x) * W), Y alike, then warp_sample_fixed's 15-bit bilinear weights on the four taps
//            (X >> 5, Y >> 5) .. + 1.  OCVAR_WARP_NEAREST: the same expressions with 1. in place of 32. (W == 0 giving 0), and the
//            pixel is the source pixel at (X, Y) = (rint(clamp(..)), rint(clamp(..))).  Every byte of a pixel is treated alike,
//            byte 3 of a four-channel pixel included.
//   border   OCVAR_WARP_BORDER_CONSTANT: a tap outside the source reads fill[c], four caller bytes in the format's memory order
//            (fill 0 is warp_sample_fixed's rule).  OCVAR_WARP_BORDER_REPLICATE: tap coordinates are clamped into the source.
//   records  the four corners of a record go through the FORWARD map in double, x' = (m0 x + m1 y + m2) / w, y' alike,
//            w = m6 x + m7 y + m8, and are rounded once to float32, a NaN stored as 0x7FC00000 (undistort_stored); a corner whose w
//            is 0 or not finite becomes NaN.  Every other field is copied; with OCVAR_WARP_POSE glMatrix is solved from the new
//            square (square_to_glmatrix with the camera of the call and the record's aspectRatio), as ocvar_hip_scale_records does.
//            Slot k of a frame is written when k < min(count, slots); the other slots are not touched.  A map the frame call would
//            skip still goes through these formulas.
//   plane    warp_board_plane_map: the destination -> source map K [r1 r2 t] S of a board pose (rvec, tvec, status), K the camera
//            matrix (all nine entries), r1 r2 the first two columns of the rotation of rvec -- pose_core.h's rodrigues_t with the policy
//            WarpSinCos: sine and cosine computed here in plain double arithmetic (warp_sincos) --, and S the map from
//            destination pixels to board units that sends pixel (0, 0) to (x0, y0) and pixel (dst_w - 1, dst_h - 1) to (x1, y1):
//            sx = (x1 - x0) / (dst_w - 1), 0 when dst_w is 1, sy alike -- the caller flips by choosing y0 > y1.  With P = K [r1 r2 t]
//            (each entry the three products summed left to right): M[3i] = P[3i] sx, M[3i+1] = P[3i+1] sy,
//            M[3i+2] = P[3i] x0 + P[3i+1] y0 + P[3i+2].  The lens is ignored: undistort the frames first.  A pose whose status is
//            not 1, a number that is not finite (inputs or result), or a rectangle of zero extent on an axis whose destination side
//            is above 1 gives nine NaNs (one fixed quiet NaN), and the warp then skips that frame.
//   plan     warp_tile_plan: how the kernel reads the source for one destination tile -- STAGED through LDS with a source window, or
//            DIRECT from global memory.  w = M[6] x + M[7] y + M[8] is linear, so when it has one sign on the tile's four corner
//            pixels it has that sign, and no zero, on the whole tile, the tile's image is the convex quad of its corners' images,
//            and the taps lie in that quad's bounding box grown by WARP_WINDOW_MARGIN; the window is that box with both ends clamped
//            into the frame (which is where REPLICATE sends the taps beyond it).  DIRECT when w changes sign or reaches 0 (or is
//            not finite) over the corners, when a corner's image is not finite or beyond WARP_PLAN_MAX_COORD, or when the window
//            exceeds the LDS budget.  THE BYTES NEVER DEPEND ON THE PLAN: a tap outside a staged window is read from global memory.
//
// All arithmetic is integer or IEEE double (-ffp-contract=off): the host build (tests/emul/warp_emul.cpp) gives the bytes of the
// kernels (warp.hip).  warp_frames and warp_records are that host reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "decode_core.h"
#include "patch_core.h"
#include "pose_core.h"
#include "tail_core.h"
#include "undistort_core.h"
#include <math.h>

namespace ocvar {

constexpr int WARP_MAX_SIDE = 32767;
constexpr int WARP_FLAGS = OCVAR_WARP_INVERSE_MAP | OCVAR_WARP_ONE_MAP;                             // of ocvar_hip_warp
constexpr int WARP_REC_FLAGS = OCVAR_WARP_INVERSE_MAP | OCVAR_WARP_ONE_MAP | OCVAR_WARP_POSE;       // known to ocvar_hip_warp_records
// The kernel's destination tile: a workgroup of 256 lanes, each 4 consecutive pixels of a row in warp_lane_rows(bpp) rows 16 apart
// (64 x 64 pixels at 1 byte per pixel, 64 x 32 at 3 and 4: the windows of both fit the LDS image), and that image in dwords: 16 KiB,
// so that the 160 KiB of a CU hold the images of as many workgroups as its wave slots take.
constexpr int WARP_TILE_W = 64, WARP_LANE_PX = 4, WARP_ROW_STEP = 16, WARP_THREADS = 256;
OCVAR_HD constexpr int warp_lane_rows(int bpp) { return bpp == 1 ? 4 : 2; }
OCVAR_HD constexpr int warp_tile_h(int bpp) { return WARP_ROW_STEP * warp_lane_rows(bpp); }
constexpr int WARP_LDS_DWORDS = 4096;
constexpr int WARP_WINDOW_MARGIN = 1;              // pixels around the corners' bounding box besides the bilinear taps' + 1
constexpr double WARP_PLAN_MAX_COORD = 1e6;        // a corner image beyond this (either sign) makes the tile direct

OCVAR_HD bool warp_interp_ok(int v) { return v == OCVAR_WARP_NEAREST || v == OCVAR_WARP_LINEAR; }
OCVAR_HD bool warp_border_ok(int v) { return v == OCVAR_WARP_BORDER_CONSTANT || v == OCVAR_WARP_BORDER_REPLICATE; }
OCVAR_HD bool warp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (a NaN fails the comparison too)

// The status rule and the destination -> source map M of one frame; false: the frame is skipped.
OCVAR_HD bool warp_map(const double* m, int flags, double* M) {
    for (int i = 0; i < 9; i++)
        if (!warp_finite(m[i])) return false;
    if (flags & OCVAR_WARP_INVERSE_MAP) {
        for (int i = 0; i < 9; i++) M[i] = m[i];
        return true;
    }
    const double* S = m;   // invert_map's formula on doubles
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (!(d != 0.) || !warp_finite(d)) return false;
    d = 1. / d;
    M[0] = (S[4] * S[8] - S[5] * S[7]) * d;
    M[1] = (S[2] * S[7] - S[1] * S[8]) * d;
    M[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    M[3] = (S[5] * S[6] - S[3] * S[8]) * d;
    M[4] = (S[0] * S[8] - S[2] * S[6]) * d;
    M[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    M[6] = (S[3] * S[7] - S[4] * S[6]) * d;
    M[7] = (S[1] * S[6] - S[0] * S[7]) * d;
    M[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    for (int i = 0; i < 9; i++)
        if (!warp_finite(M[i])) return false;
    return true;
}

// The source position of destination pixel (x, y) in units of 1 / scale pixels (scale 32: LINEAR, 1: NEAREST): warp_sample_px's
// expressions.
OCVAR_HD void warp_source_fixed(const double* M, int x, int y, double scale, int* X, int* Y) {
    const double X0 = M[0] * 0 + M[1] * y + M[2];
    const double Y0 = M[3] * 0 + M[4] * y + M[5];
    const double W0 = M[6] * 0 + M[7] * y + M[8];
    double W = W0 + M[6] * x;
    W = W ? scale / W : 0;
    *X = warp_fixed32((X0 + M[0] * x) * W);
    *Y = warp_fixed32((Y0 + M[3] * x) * W);
}

// One tap under the border rule: px(ix, iy) is called for pixels inside the cw x ch source only.
template <class Px>
OCVAR_HD int warp_tap(Px px, int cw, int ch, int ix, int iy, int border, int fill) {
    if (border == OCVAR_WARP_BORDER_REPLICATE) {
        ix = ix < 0 ? 0 : (ix > cw - 1 ? cw - 1 : ix);
        iy = iy < 0 ? 0 : (iy > ch - 1 ? ch - 1 : iy);
        return px(ix, iy);
    }
    return (ix >= 0 && ix < cw && iy >= 0 && iy < ch) ? px(ix, iy) : fill;
}

// warp_sample_fixed's weights of the fractions (fx, fy), 1/32 px each
OCVAR_HD void warp_weights(int fx, int fy, int* w) {
    w[0] = (32 - fx) * (32 - fy) * 32;
    w[1] = fx * (32 - fy) * 32;
    w[2] = (32 - fx) * fy * 32;
    w[3] = fx * fy * 32;
    if ((fx | fy) == 0) {
        w[0] = 32767;
        w[3] = 1;
    }
}

// warp_sample_fixed with the border rule and the fill: with CONSTANT and fill 0 the same number.
template <class Px>
OCVAR_HD int warp_sample_linear(Px px, int cw, int ch, int X, int Y, int border, int fill) {
    int ix = X >> 5, iy = Y >> 5;
    ix = ix > 32767 ? 32767 : (ix < -32768 ? -32768 : ix);
    iy = iy > 32767 ? 32767 : (iy < -32768 ? -32768 : iy);
    int w[4];
    warp_weights(X & 31, Y & 31, w);
    const int p00 = warp_tap(px, cw, ch, ix, iy, border, fill), p01 = warp_tap(px, cw, ch, ix + 1, iy, border, fill);
    const int p10 = warp_tap(px, cw, ch, ix, iy + 1, border, fill), p11 = warp_tap(px, cw, ch, ix + 1, iy + 1, border, fill);
    return (p00 * w[0] + p01 * w[1] + p10 * w[2] + p11 * w[3] + 16384) >> 15;
}

// Byte c of the destination pixel whose source position is (X, Y) (warp_source_fixed with the interpolation's scale).
template <class Px>
OCVAR_HD int warp_sample(Px px, int cw, int ch, int X, int Y, int interp, int border, int fill) {
    return interp == OCVAR_WARP_LINEAR ? warp_sample_linear(px, cw, ch, X, Y, border, fill) : warp_tap(px, cw, ch, X, Y, border, fill);
}
OCVAR_HD double warp_scale(int interp) { return interp == OCVAR_WARP_LINEAR ? 32. : 1.; }

// One launch's arguments, all pointers in device memory: frame f's pixels start *_frame_stride bytes after frame f - 1's, rows
// *_row_stride apart; the two sides do not overlap.  maps: [n][9] doubles, or [9] with OCVAR_WARP_ONE_MAP in flags; status [n] or
// nullptr.  direct: a tuning switch, every tile takes the direct class (the bytes are the same).
struct WarpArgs {
    const uint8_t* src;
    uint8_t* dst;
    int sw, sh, dw, dh;
    long long src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride;
    const double* maps;
    int* status;
    int interp, border, flags, direct;
    uint8_t fill[4];
};

OCVAR_HD const double* warp_frame_map(const WarpArgs& a, int f) { return (a.flags & OCVAR_WARP_ONE_MAP) ? a.maps : a.maps + 9 * (long long)f; }

// ---- the tile plan ---------------------------------------------------------------------------------------------------------------

// The class of one destination tile and, when staged, its source window: pixels x0 .. x0 + w - 1, rows y0 .. y0 + h - 1, all inside
// the frame; its LDS image holds the bytes from byte b0 (a multiple of 4) of those rows, `pitch` dwords per row.
struct WarpPlan {
    int staged;
    int x0, y0, w, h;
    int b0, row_dwords, pitch;
};

// The tile's pixels are (tx0 .. tx0 + tw - 1) x (ty0 .. ty0 + th - 1), tw, th >= 1; the source is sw x sh at bpp bytes per pixel.
OCVAR_HD WarpPlan warp_tile_plan(const double* M, int tx0, int ty0, int tw, int th, int sw, int sh, int bpp, int interp, int budget_dwords) {
    WarpPlan p{};
    double umin = 0, umax = 0, vmin = 0, vmax = 0;
    int sign = 0;
    for (int k = 0; k < 4; k++) {
        const double x = (double)((k == 1 || k == 2) ? tx0 + tw - 1 : tx0), y = (double)(k >= 2 ? ty0 + th - 1 : ty0);
        const double w = M[6] * x + M[7] * y + M[8];
        if (!warp_finite(w) || w == 0.) return p;
        const int s = w > 0. ? 1 : -1;
        if (k && s != sign) return p;
        sign = s;
        const double iw = 1. / w, u = (M[0] * x + M[1] * y + M[2]) * iw, v = (M[3] * x + M[4] * y + M[5]) * iw;
        if (!(fabs(u) <= WARP_PLAN_MAX_COORD) || !(fabs(v) <= WARP_PLAN_MAX_COORD)) return p;
        umin = (k == 0 || u < umin) ? u : umin;
        umax = (k == 0 || u > umax) ? u : umax;
        vmin = (k == 0 || v < vmin) ? v : vmin;
        vmax = (k == 0 || v > vmax) ? v : vmax;
    }
    // LINEAR reads floor(u) and floor(u) + 1, NEAREST rint(u); the margin covers the roundings of the two ways to the same number
    const int far = interp == OCVAR_WARP_LINEAR ? 1 : 0;
    int x0 = (int)floor(umin) - WARP_WINDOW_MARGIN, x1 = (int)floor(umax) + 1 + far + WARP_WINDOW_MARGIN;
    int y0 = (int)floor(vmin) - WARP_WINDOW_MARGIN, y1 = (int)floor(vmax) + 1 + far + WARP_WINDOW_MARGIN;
    x0 = x0 < 0 ? 0 : (x0 > sw - 1 ? sw - 1 : x0);
    x1 = x1 < 0 ? 0 : (x1 > sw - 1 ? sw - 1 : x1);
    y0 = y0 < 0 ? 0 : (y0 > sh - 1 ? sh - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > sh - 1 ? sh - 1 : y1);
    p.x0 = x0;
    p.y0 = y0;
    p.w = x1 - x0 + 1;
    p.h = y1 - y0 + 1;
    p.b0 = (x0 * bpp) & ~3;
    p.row_dwords = ((x1 + 1) * bpp + 3 - p.b0) >> 2;
    p.pitch = (p.row_dwords + 1) | 1;      // odd, and one spare dword: a lane's aligned reads run up to 2 dwords past a pixel's first
    // (the image's last two dwords are spare for the same reason)
    p.staged = (long long)p.h * p.pitch + 2 <= (long long)budget_dwords;
    return p;
}

// ---- the host reference -------------------------------------------------------------------------------------------------------------

// Frame f of the launch in format fmt, sequentially: its status (when asked for) and, unless it is skipped, its pixels.
inline int warp_frame(const WarpArgs& a, int fmt, int f) {
    const int bpp = format_bpp(fmt);
    double M[9];
    const bool ok = warp_map(warp_frame_map(a, f), a.flags, M);
    if (a.status) a.status[f] = ok ? 1 : 0;
    if (!ok) return 0;
    const uint8_t* src = a.src + (long long)f * a.src_frame_stride;
    uint8_t* dst = a.dst + (long long)f * a.dst_frame_stride;
    const long long rs = a.src_row_stride;
    for (int y = 0; y < a.dh; y++)
        for (int x = 0; x < a.dw; x++) {
            int X, Y;
            warp_source_fixed(M, x, y, warp_scale(a.interp), &X, &Y);
            for (int c = 0; c < bpp; c++)
                dst[(long long)y * a.dst_row_stride + (long long)x * bpp + c] = (uint8_t)warp_sample(
                    [=](int ix, int iy) -> int { return src[(long long)iy * rs + (long long)ix * bpp + c]; }, a.sw, a.sh, X, Y, a.interp, a.border, a.fill[c]);
        }
    return 1;
}
inline int warp_frames(const WarpArgs& a, int fmt, int n_frames) {
    int done = 0;
    for (int f = 0; f < n_frames; f++) done += warp_frame(a, fmt, f);
    return done;
}

// ---- records ------------------------------------------------------------------------------------------------------------------------

// The record map on one square (8 floats; out may be sq) under the forward map m.
OCVAR_HD void warp_square(const double* m, const float* sq, float* out) {
    for (int k = 0; k < 4; k++) {
        const double x = sq[2 * k], y = sq[2 * k + 1];
        const double w = m[6] * x + m[7] * y + m[8];
        if (!warp_finite(w) || w == 0.) {
            out[2 * k] = out[2 * k + 1] = __builtin_nanf("");
        } else {
            const double xo = (m[0] * x + m[1] * y + m[2]) / w, yo = (m[3] * x + m[4] * y + m[5]) / w;
            out[2 * k] = undistort_stored(xo);
            out[2 * k + 1] = undistort_stored(yo);
        }
    }
}

OCVAR_HD void warp_record(MarkerRec& r, const double* m, int flags, const CameraRec& cam) {
    warp_square(m, r.square, r.square);
    if (flags & OCVAR_WARP_POSE) {
        double gl[16];
        square_to_glmatrix(r.square, cam, r.aspectRatio, gl);
        for (int q = 0; q < 16; q++) r.glMatrix[q] = gl[q];
    }
}

// The host reference of the record call: slots k < min(count, slots) of one frame from in to out (which may be the same array).
inline int warp_records(const MarkerRec* in, int count, int slots, const double* m, int flags, const CameraRec& cam, MarkerRec* out) {
    const int n = count < slots ? count : slots;
    for (int k = 0; k < n; k++) {
        MarkerRec r = in[k];
        warp_record(r, m, flags, cam);
        out[k] = r;
    }
    return n < 0 ? 0 : n;
}

// ---- the board's plane ----------------------------------------------------------------------------------------------------------------

// Sine and cosine of theta >= 0 in additions and multiplications of doubles only, so that host and device give the same bits: the
// two math libraries differ in the last bit of sin and cos for about one angle in fifteen (5 of 71 test poses), and a map decides
// bytes.  Cody-Waite reduction by pi / 2 in two parts (33 + 53 bits: exact products below 2^20 quarter turns; an rvec is at most pi
// long) and fdlibm's kernel polynomials on [-pi / 4, pi / 4]; within 1 ulp of the true values there.
OCVAR_HD void warp_sincos(double theta, double* s, double* c) {
    const double fn = rint(theta * 6.36619772367581382433e-01);
    const double r = theta - fn * 1.57079632673412561417e+00, w = fn * 6.07710050650619224932e-11;
    const double x = r - w, y = (r - x) - w;      // x + y: theta less fn quarter turns
    const double z = x * x, v = z * x;
    const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    const double ks = x - ((z * (0.5 * y - v * rs) - y) - v * -1.66666666666666324348e-01);
    const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double kc = 1.0 - (0.5 * z - (z * rc - x * y));
    const int q = (int)fmod(fn, 4.0);
    *s = q == 0 ? ks : (q == 1 ? kc : (q == 2 ? -ks : -kc));
    *c = q == 0 ? kc : (q == 1 ? -ks : (q == 2 ? -kc : ks));
}

// rodrigues_t's policy (pose_core.h) that takes them from there
struct WarpSinCos {
    static OCVAR_HD void at(double theta, double* s, double* c) { warp_sincos(theta, s, c); }
};

// The destination -> source map of the rectangle rect = (x0, y0, x1, y1) of a board's plane seen by camera matrix K under the pose,
// for a destination of dw x dh pixels; nine NaNs when there is none.
OCVAR_HD void warp_board_plane_map(const OcvarBoardPose& pose, const double* K, const double* rect, int dw, int dh, double* M) {
    const double nan = __builtin_nan("");
    bool ok = pose.status == 1;
    for (int i = 0; i < 3; i++) ok = ok && warp_finite(pose.rvec[i]) && warp_finite(pose.tvec[i]);
    for (int i = 0; i < 9; i++) ok = ok && warp_finite(K[i]);
    for (int i = 0; i < 4; i++) ok = ok && warp_finite(rect[i]);
    ok = ok && !(dw > 1 && rect[2] - rect[0] == 0.) && !(dh > 1 && rect[3] - rect[1] == 0.);
    if (ok) {
        double R[9];
        rodrigues_t<false, WarpSinCos>(pose.rvec, R, nullptr);
        const double A[9] = {R[0], R[1], pose.tvec[0], R[3], R[4], pose.tvec[1], R[6], R[7], pose.tvec[2]};   // [r1 r2 t]
        const double sx = dw > 1 ? (rect[2] - rect[0]) / (double)(dw - 1) : 0., sy = dh > 1 ? (rect[3] - rect[1]) / (double)(dh - 1) : 0.;
        for (int i = 0; i < 3; i++) {
            const double p0 = K[3 * i] * A[0] + K[3 * i + 1] * A[3] + K[3 * i + 2] * A[6];
            const double p1 = K[3 * i] * A[1] + K[3 * i + 1] * A[4] + K[3 * i + 2] * A[7];
            const double p2 = K[3 * i] * A[2] + K[3 * i + 1] * A[5] + K[3 * i + 2] * A[8];
            M[3 * i] = p0 * sx;
            M[3 * i + 1] = p1 * sy;
            M[3 * i + 2] = p0 * rect[0] + p1 * rect[1] + p2;
        }
        for (int i = 0; i < 9; i++) ok = ok && warp_finite(M[i]);
    }
    if (!ok)
        for (int i = 0; i < 9; i++) M[i] = nan;
}

}  // namespace ocvar

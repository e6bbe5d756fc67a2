// undistort_core.h -- frames and marker records of a distorting camera turned into the pinhole world of the same camera matrix,
// on frames and records that stay in device memory (opt-in: ocvar_hip_undistort / ocvar_hip_undistort_records).  Frames: OpenCV's
// undistort(src, dst, cameraMatrix, distCoeffs, newCameraMatrix = cameraMatrix) with bilinear sampling and a constant 0 border;
// record corners: undistortPoints(square, cameraMatrix, distCoeffs, R = I, P = cameraMatrix).  Afterwards glProjection (a pinhole
// projection), the overlays' homographies and the patches' straight-edged quads are exact on what the caller shows.  No
// counterpart in the reference, which draws the distorted frame behind a pinhole rendering.
//
// Camera: fx, fy, cx, cy = cameraMatrix[0], [4], [2], [5]; dist = distCoeffs = k1 k2 p1 p2 k3.
//   frame    destination pixel (u, v) reads the source at (us, vs) = undistort_source(cam, u, v): the lens model applied to the
//            pixel's normalised point, in this order and no other:
//              x = (u - cx) * (1 / fx), y = (v - cy) * (1 / fy)                       (board_undistort_t<false>)
//              r2 = x * x + y * y, cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
//              xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)                   (C's left-to-right evaluation)
//              yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
//              us = fx * xd + cx, vs = fy * yd + cy
//            X = warp_fixed32(32 * us), Y = warp_fixed32(32 * vs), and byte c of the pixel is warp_sample_fixed(px_c, W, H, X, Y)
//            of decode_core.h: cvWarpPerspective's 1/32-px bilinear sampling with 15-bit weights, 0 outside the frame.  Every
//            byte of a pixel is remapped alike, byte 3 of a four-channel pixel included (as patch_core.h).  With all five
//            coefficients zero (us, vs) is (u, v) up to a few roundings of doubles, X = 32 u and Y = 32 v for any camera that
//            keeps those roundings below 1/64 px, and the sampler's exact-position weights (32767, 1) return the source byte:
//            the frame is copied.
//   record   corner (u, v) of `square` becomes (x * fx + cx, y * fy + cy) rounded to float32, (x, y) = board_undistort_t<true>:
//            cvUndistortPoints' five fixed-point iterations.  When all five coefficients are exactly zero the square is copied
//            unchanged (a rule of its own, so that the result is exact).  Every other field of the record is copied as it is,
//            glMatrix included: the distortion-aware pose is the physical pose, and its pinhole projection with cameraMatrix
//            lands on the undistorted corners.  Non-finite coordinates give whatever the formulas give; a coordinate that comes
//            out as a NaN is stored as the quiet NaN 0x7FC00000 (sign and payload of a computed NaN are the processor's choice).
//            Slot k of a frame is written when k < min(count, slots); the other slots are not touched.
//
// All arithmetic is integer or IEEE double (-ffp-contract=off): the host build (tests/emul/undistort_emul.cpp) gives the bytes of
// the kernels (undistort.hip).  undistort_frame and undistort_records are that host reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "decode_core.h"
#include "tail_core.h"
#include "board_core.h"
#include "patch_core.h"
#include <math.h>

namespace ocvar {

// the nine numbers of a camera the maps use; passed by value in the launch arguments
struct UndistortCam {
    double fx, fy, cx, cy;
    double dist[5];
};

OCVAR_HD UndistortCam undistort_cam(const CameraRec& c) {
    UndistortCam u;
    u.fx = c.cameraMatrix[0];
    u.fy = c.cameraMatrix[4];
    u.cx = c.cameraMatrix[2];
    u.cy = c.cameraMatrix[5];
    for (int i = 0; i < 5; i++) u.dist[i] = c.distCoeffs[i];
    return u;
}

// what the entry points ask of a camera: nine finite numbers, focal lengths that are not zero
inline bool undistort_cam_ok(const UndistortCam& c) {
    for (int i = 0; i < 5; i++)
        if (!isfinite(c.dist[i])) return false;
    return isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy) && c.fx != 0.0 && c.fy != 0.0;
}

OCVAR_HD bool undistort_no_lens(const UndistortCam& c) {
    return c.dist[0] == 0.0 && c.dist[1] == 0.0 && c.dist[2] == 0.0 && c.dist[3] == 0.0 && c.dist[4] == 0.0;
}

// The frame map: where in the source (pixels) destination position (u, v) is read (the kernels pass whole pixels).
OCVAR_HD void undistort_source(const UndistortCam& c, double u, double v, double* us, double* vs) {
    double n[2];
    board_undistort_t<false>(u, v, c.fx, c.fy, c.cx, c.cy, c.dist, n);
    const double x = n[0], y = n[1];
    const double r2 = x * x + y * y;
    const double cd = 1 + ((c.dist[4] * r2 + c.dist[1]) * r2 + c.dist[0]) * r2;
    const double xd = x * cd + 2 * c.dist[2] * x * y + c.dist[3] * (r2 + 2 * x * x);
    const double yd = y * cd + c.dist[2] * (r2 + 2 * y * y) + 2 * c.dist[3] * x * y;
    *us = c.fx * xd + c.cx;
    *vs = c.fy * yd + c.cy;
}

// the same in the sampler's fixed point, 1/32 px
OCVAR_HD void undistort_source_fixed(const UndistortCam& c, int u, int v, int* X, int* Y) {
    double us, vs;
    undistort_source(c, (double)u, (double)v, &us, &vs);
    *X = warp_fixed32(32 * us);
    *Y = warp_fixed32(32 * vs);
}

// Byte ch of the destination pixel whose source position is (X, Y), from a W x H frame of bpp bytes per pixel, rows row_stride
// bytes apart.
OCVAR_HD int undistort_sample(const uint8_t* frame, int W, int H, long long row_stride, int bpp, int ch, int X, int Y) {
    return warp_sample_fixed([=](int ix, int iy) -> int { return frame[(long long)iy * row_stride + (long long)ix * bpp + ch]; }, W, H, X, Y);
}

// a float32 result as it is stored: itself, or the one NaN of the definition
OCVAR_HD float undistort_stored(double v) {
    const float r = (float)v;
    return r != r ? __builtin_nanf("") : r;
}

// The record map on one square (8 floats; out may be sq).
OCVAR_HD void undistort_square(const UndistortCam& c, const float* sq, float* out) {
    if (undistort_no_lens(c)) {
        for (int i = 0; i < 8; i++) out[i] = sq[i];
        return;
    }
    for (int k = 0; k < 4; k++) {
        double n[2];
        board_undistort_t<true>((double)sq[2 * k], (double)sq[2 * k + 1], c.fx, c.fy, c.cx, c.cy, c.dist, n);
        out[2 * k] = undistort_stored(n[0] * c.fx + c.cx);
        out[2 * k + 1] = undistort_stored(n[1] * c.fy + c.cy);
    }
}

// The host reference of the frame map: one W x H frame in format fmt from src to dst (which do not overlap), sequentially.
inline void undistort_frame(const uint8_t* src, int W, int H, long long src_row_stride, int fmt, const UndistortCam& cam, uint8_t* dst,
                            long long dst_row_stride) {
    const int bpp = format_bpp(fmt);
    for (int v = 0; v < H; v++)
        for (int u = 0; u < W; u++) {
            int X, Y;
            undistort_source_fixed(cam, u, v, &X, &Y);
            for (int ch = 0; ch < bpp; ch++)
                dst[(long long)v * dst_row_stride + (long long)u * bpp + ch] = (uint8_t)undistort_sample(src, W, H, src_row_stride, bpp, ch, X, Y);
        }
}

// The host reference of the record map: slots k < min(count, slots) of one frame from in to out (which may be the same array).
// Returns the number of slots written.
inline int undistort_records(const UndistortCam& cam, const MarkerRec* in, int count, int slots, MarkerRec* out) {
    const int n = count < slots ? count : slots;
    for (int k = 0; k < n; k++) {
        MarkerRec r = in[k];
        undistort_square(cam, r.square, r.square);
        out[k] = r;
    }
    return n < 0 ? 0 : n;
}

}  // namespace ocvar

// orient_core.h -- device-resident frames turned and mirrored, marker records carried between the two orientations, and the camera
// that belongs to the turned frames (opt-in: ocvar_hip_orient / ocvar_hip_orient_records / ocvar_hip_orient_camera).  A sideways
// camera, a clip with a 90 degree display matrix or a mirrored front camera is turned upright before it is detected -- the
// reference's registration is not invariant to the frame's orientation --, and the records found there are carried back to the
// frames as they were delivered.  The reference has nothing of the kind.
//
// The frame step is a pure permutation of pixels: OpenCV's rotate, flip and transpose cannot differ from it.  The eight
// orientations are the symmetries of the rectangle.  A source pixel or coordinate (x, y) of a W x H frame goes to (x', y'):
//   OCVAR_ORIENT_IDENTITY    x' = x          y' = y          W x H   copy
//   OCVAR_ORIENT_ROT90_CW    x' = H - 1 - y  y' = x          H x W   rotate(ROTATE_90_CLOCKWISE)
//   OCVAR_ORIENT_ROT180      x' = W - 1 - x  y' = H - 1 - y  W x H   rotate(ROTATE_180)
//   OCVAR_ORIENT_ROT270_CW   x' = y          y' = W - 1 - x  H x W   rotate(ROTATE_90_COUNTERCLOCKWISE)
//   OCVAR_ORIENT_FLIP_H      x' = W - 1 - x  y' = y          W x H   flip(1)
//   OCVAR_ORIENT_FLIP_V      x' = x          y' = H - 1 - y  W x H   flip(0)
//   OCVAR_ORIENT_TRANSPOSE   x' = y          y' = x          H x W   transpose
//   OCVAR_ORIENT_TRANSVERSE  x' = H - 1 - y  y' = W - 1 - x  H x W   transpose of flip(-1)
// The inverse of ROT90_CW is ROT270_CW and the other way round; every other orientation is its own inverse.  TRANSPOSE is FLIP_H
// after ROT90_CW, TRANSVERSE is FLIP_V after ROT90_CW.
//   records  each of the four corners goes through the table in double and is rounded to float32, a NaN stored as 0x7FC00000
//            (undistort_core.h: undistort_stored); a coordinate that the table passes through unchanged, or only swaps between the
//            axes, is copied bit for bit.  Corner k stays in slot k, so FLIP_H, FLIP_V, TRANSPOSE and TRANSVERSE -- the mirroring
//            orientations -- REVERSE THE WINDING of the square: a square that ran clockwise on screen runs counter-clockwise
//            afterwards.  Every other field is copied.  With OCVAR_ORIENT_POSE glMatrix is solved from the new square
//            (square_to_glmatrix with the camera of the call -- that of the destination orientation: orient_camera -- and the
//            record's aspectRatio); a reflected view has no rigid pose, so the flag is refused for the mirroring orientations.
//            Slot k of a frame is written when k < min(count, slots); the other slots are not touched.
//   pose     under a rotation the camera frame turns about the optical axis with the picture.  With M the 4 x 4 matrix glMatrix
//            holds column by column (gl_from_pose: its upper 3 x 3 is F R F, its last column F t, F = diag(1, 1, -1), which
//            commutes with a turn about z), the pose of the turned square under the turned camera is Z M, Z the turn of the
//            normalised image plane:  ROT90_CW  x' = -y, y' = x  (rows 0 and 1 of M become -row 1 and row 0: +90 degrees about
//            the optical axis, x towards y);  ROT180  x' = -x, y' = -y;  ROT270_CW  x' = y, y' = -x.
//   camera   width and height are the destination's; fx and fy swap when the orientation transposes; the principal point goes
//            through the table in double (cx' = H - 1 - cy for ROT90_CW: pixel centres lie on integers); glProjection is computed
//            from those as cvarCameraScale does.  Of the distortion coefficients k1 k2 p1 p2 k3 the radial ones are kept, and
//            with dx = 2 p1 x y + p2 (r^2 + 2 x^2), dy = p1 (r^2 + 2 y^2) + 2 p2 x y the tangential pair (p1, p2) becomes
//              ROT90_CW (p2, -p1)   ROT180 (-p1, -p2)   ROT270_CW (-p2, p1)   FLIP_H (p1, -p2)   FLIP_V (-p1, p2)
//              TRANSPOSE (p2, p1)   TRANSVERSE (-p2, -p1)
//            so that distorting a point and turning the pixel equals turning the point and distorting it under the new camera.
//            A camera matrix that is not fx 0 cx / 0 fy cy / 0 0 1 (skew, for one) is refused for every orientation but IDENTITY,
//            which keeps everything but glProjection.
//
// Nothing here rounds but the records' float32: the host build (tests/emul/orient_emul.cpp) gives the bytes of the kernels
// (orient.hip).  orient_frame and orient_records are that host reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "patch_core.h"
#include "pose_core.h"
#include "tail_core.h"
#include "undistort_core.h"

namespace ocvar {

constexpr int ORIENT_MAX_SIDE = 32767;
constexpr int ORIENT_FLAGS = OCVAR_ORIENT_POSE;

OCVAR_HD bool orient_ok(int o) { return o >= OCVAR_ORIENT_IDENTITY && o <= OCVAR_ORIENT_TRANSVERSE; }
// the destination is H x W
OCVAR_HD bool orient_transposes(int o) { return o == OCVAR_ORIENT_ROT90_CW || o == OCVAR_ORIENT_ROT270_CW || o >= OCVAR_ORIENT_TRANSPOSE; }
// a reflection: the winding of a square is reversed
OCVAR_HD bool orient_mirrors(int o) { return o >= OCVAR_ORIENT_FLIP_H; }
OCVAR_HD int orient_inverse(int o) { return o == OCVAR_ORIENT_ROT90_CW ? OCVAR_ORIENT_ROT270_CW : (o == OCVAR_ORIENT_ROT270_CW ? OCVAR_ORIENT_ROT90_CW : o); }
OCVAR_HD int orient_dst_width(int o, int W, int H) { return orient_transposes(o) ? H : W; }
OCVAR_HD int orient_dst_height(int o, int W, int H) { return orient_transposes(o) ? W : H; }
// x' (y') counts down from the far end of the SOURCE axis it is taken from
OCVAR_HD bool orient_reverses_x(int o) {
    return o == OCVAR_ORIENT_ROT90_CW || o == OCVAR_ORIENT_ROT180 || o == OCVAR_ORIENT_FLIP_H || o == OCVAR_ORIENT_TRANSVERSE;
}
OCVAR_HD bool orient_reverses_y(int o) {
    return o == OCVAR_ORIENT_ROT180 || o == OCVAR_ORIENT_ROT270_CW || o == OCVAR_ORIENT_FLIP_V || o == OCVAR_ORIENT_TRANSVERSE;
}

// The table on a point, in double: (x, y) of a W x H frame -> (xo, yo).
OCVAR_HD void orient_point(int o, int W, int H, double x, double y, double* xo, double* yo) {
    const double u = orient_transposes(o) ? y : x, v = orient_transposes(o) ? x : y;              // what x' and y' are taken from
    const double ue = orient_transposes(o) ? (double)(H - 1) : (double)(W - 1), ve = orient_transposes(o) ? (double)(W - 1) : (double)(H - 1);
    *xo = orient_reverses_x(o) ? ue - u : u;
    *yo = orient_reverses_y(o) ? ve - v : v;
}

// The source pixel (sx, sy) of destination pixel (dx, dy), W x H the SOURCE: what the kernels and orient_frame share.
OCVAR_HD void orient_source_index(int o, int W, int H, int dx, int dy, int* sx, int* sy) {
    if (orient_transposes(o)) {     // x' came from y, y' from x
        *sy = orient_reverses_x(o) ? H - 1 - dx : dx;
        *sx = orient_reverses_y(o) ? W - 1 - dy : dy;
    } else {
        *sx = orient_reverses_x(o) ? W - 1 - dx : dx;
        *sy = orient_reverses_y(o) ? H - 1 - dy : dy;
    }
}

// One launch's arguments, all pointers in device memory: frame f's pixels start *_frame_stride bytes after frame f - 1's, rows
// *_row_stride apart; sw x sh is the source, the destination's size follows from the orientation; the two do not overlap.
struct OrientArgs {
    const uint8_t* src;
    uint8_t* dst;
    int sw, sh;
    long long src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride;
    int orientation;
};

// The host reference of the frame call: frame f of the launch in format fmt, sequentially.
inline void orient_frame(const OrientArgs& a, int fmt, int f) {
    const int bpp = format_bpp(fmt);
    const int dw = orient_dst_width(a.orientation, a.sw, a.sh), dh = orient_dst_height(a.orientation, a.sw, a.sh);
    const uint8_t* src = a.src + (long long)f * a.src_frame_stride;
    uint8_t* dst = a.dst + (long long)f * a.dst_frame_stride;
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int sx, sy;
            orient_source_index(a.orientation, a.sw, a.sh, x, y, &sx, &sy);
            for (int c = 0; c < bpp; c++)
                dst[(long long)y * a.dst_row_stride + (long long)x * bpp + c] = src[(long long)sy * a.src_row_stride + (long long)sx * bpp + c];
        }
}

// The record map on one square (8 floats; out may be sq): a coordinate the table only passes on is copied, the others are
// (extent - 1) - p in double, rounded once.
OCVAR_HD void orient_square(const float* sq, int W, int H, int o, float* out) {
    const bool t = orient_transposes(o), rx = orient_reverses_x(o), ry = orient_reverses_y(o);
    const double ue = t ? (double)(H - 1) : (double)(W - 1), ve = t ? (double)(W - 1) : (double)(H - 1);
    for (int k = 0; k < 4; k++) {
        const float x = sq[2 * k], y = sq[2 * k + 1];
        const float u = t ? y : x, v = t ? x : y;
        out[2 * k] = rx ? undistort_stored(ue - (double)u) : u;
        out[2 * k + 1] = ry ? undistort_stored(ve - (double)v) : v;
    }
}

// One record as the call leaves it (flags and orientation as the entry point admits them: no OCVAR_ORIENT_POSE when mirroring).
OCVAR_HD void orient_record(MarkerRec& r, int W, int H, int o, int flags, const CameraRec& cam) {
    orient_square(r.square, W, H, o, r.square);
    if (flags & OCVAR_ORIENT_POSE) {
        double gl[16];
        square_to_glmatrix(r.square, cam, r.aspectRatio, gl);
        for (int q = 0; q < 16; q++) r.glMatrix[q] = gl[q];
    }
}

// The host reference of the record call: slots k < min(count, slots) of one frame from in to out (which may be the same array).
// Returns the number of slots written.
inline int orient_records(const MarkerRec* in, int count, int slots, int W, int H, int o, int flags, const CameraRec& cam, MarkerRec* out) {
    const int n = count < slots ? count : slots;
    for (int k = 0; k < n; k++) {
        MarkerRec r = in[k];
        orient_record(r, W, H, o, flags, cam);
        out[k] = r;
    }
    return n < 0 ? 0 : n;
}

// glProjection from width, height and the camera matrix: cvarCameraProjection(glstyle = 0), transposed, as cvarReadCamera and
// cvarCameraScale store it.
inline void orient_gl_projection(CameraRec& c) {
    const double nearplane = 0.1, farplane = 5000.0;
    for (int k = 0; k < 16; k++) c.glProjection[k] = 0.0;
    c.glProjection[0] = 2. * c.cameraMatrix[0] / c.width;
    c.glProjection[5] = 2. * c.cameraMatrix[4] / c.height;
    c.glProjection[8] = 2. * (c.cameraMatrix[2] / c.width) - 1.;
    c.glProjection[9] = 2. * (c.cameraMatrix[5] / c.height) - 1.;
    c.glProjection[10] = -(farplane + nearplane) / (farplane - nearplane);
    c.glProjection[14] = -2. * farplane * nearplane / (farplane - nearplane);
    c.glProjection[11] = -1;
}

// The camera of the frames orient_frame makes from the frames of `in` (out may be in).  False, and nothing written, for an
// unknown orientation or a camera matrix that is not fx 0 cx / 0 fy cy / 0 0 1 under any orientation but IDENTITY.
inline bool orient_camera(const CameraRec& in, int o, CameraRec* out) {
    if (!orient_ok(o)) return false;
    const double* K = in.cameraMatrix;
    if (o != OCVAR_ORIENT_IDENTITY && (K[1] != 0 || K[3] != 0 || K[6] != 0 || K[7] != 0 || K[8] != 1)) return false;
    CameraRec c = in;
    c.width = orient_dst_width(o, in.width, in.height);
    c.height = orient_dst_height(o, in.width, in.height);
    c.cameraMatrix[0] = orient_transposes(o) ? K[4] : K[0];
    c.cameraMatrix[4] = orient_transposes(o) ? K[0] : K[4];
    orient_point(o, in.width, in.height, K[2], K[5], &c.cameraMatrix[2], &c.cameraMatrix[5]);
    const double p1 = in.distCoeffs[2], p2 = in.distCoeffs[3];
    // the tangential pair turns like a vector (p2, p1) of the image plane: swapped by a transposition, negated with its axis
    const double a = orient_transposes(o) ? p2 : p1, b = orient_transposes(o) ? p1 : p2;
    c.distCoeffs[2] = orient_reverses_y(o) ? -a : a;
    c.distCoeffs[3] = orient_reverses_x(o) ? -b : b;
    orient_gl_projection(c);
    *out = c;
    return true;
}

}  // namespace ocvar

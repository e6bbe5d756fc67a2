// board_core.h -- one rigid pose of a planar marker board from every board marker a frame's records hold (opt-in:
// ocvar_hip_set_board).  ArUco's estimatePoseBoard / ARToolKit's multi-marker set; no counterpart in the reference.
//
// Per frame:
//   choose    every record with score > 0 whose template is square and on the board (map: templateId -> board index); of
//             each board entry the first such record in output order
//   rotate    the chosen record's code is read again on the frame's grey image at the record's own square, with decode's
//             readout (perspective_from_quad / invert_map / warp_sample_px / code_cell, as read_code); bit == code[k] says that
//             board corner c is record corner (c + k) & 3 (k = 0: corner c is where the code[0] readout puts corner c of its
//             destination rectangle); no k: the marker is not used.  Tracked and new records alike.
//   seed      from each of the (up to) BOARD_SEEDS used markers of largest image area (ties: the lower board index): that
//             marker's 4-point homography board plane -> undistorted normalised points, decomposed as square_to_glmatrix_t
//   refine    Levenberg-Marquardt over all 4 n corners, pose_core's CvLevMarq schedule (lambda 1e-3, 20 iterations, FLT_EPSILON
//             relative step); the seed with the lowest final error wins (ties: the earlier seed)
// The summation order is part of the definition, so that the host build (tests/emul/board_emul.cpp) reproduces the device's
// selection and counts bit for bit and its poses up to the last bits of device libm: BOARD_LANES lanes share the corners,
// lane l takes corners l, l + 64, ... (corner j = observation j / 4, board corner j % 4) in that order, and the 64 partial sums
// combine in the tree board_tree spells out (lane l + lane l ^ 32, then ^ 16, ... ^ 1: the butterfly of board_pose_kernel
// leaves that value in every lane).
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "decode_core.h"
#include "pose_core.h"
#include "tail_core.h"
#include <float.h>
#include <math.h>

namespace ocvar {

constexpr int BOARD_MAX = OCVAR_MAX_BOARD_MARKERS;
constexpr int BOARD_LANES = 64;
constexpr int BOARD_SEEDS = 4;
constexpr int BOARD_SUMS = 28;   // J^T J (upper triangle, row-major: 21), J^T e (6), e^T e (1)

struct BoardEntry {   // == OcvarBoardMarker, 72 bytes
    int templateId;
    int pad;
    double corner[8];   // board plane (z = 0) coordinates of corners 0..3
};

struct BoardPose {    // == OcvarBoardPose, 192 bytes
    double glMatrix[16];
    double rvec[3], tvec[3];
    double rms;
    int n_markers;
    int status;       // 1 solved, 0 no board marker, -1 not solvable
};

// One used marker: its board index and its image corners in BOARD corner order.  T = float on the device (record squares); the
// host build also takes double observations (tests of the solver alone).
template <class T>
struct BoardObsT {
    int index;
    T sq[8];
};
using BoardObs = BoardObsT<float>;   // 36 bytes

// ---- set_board's rules (host) ------------------------------------------------------------------------------------------------

// a convex quad of non-zero area with finite corners: the four turns have one strict sign
inline bool board_quad_ok(const double* q) {
    for (int k = 0; k < 8; k++)
        if (!isfinite(q[k])) return false;
    int pos = 0, neg = 0;
    for (int i = 0; i < 4; i++) {
        const double* a = q + 2 * i;
        const double* b = q + 2 * ((i + 1) & 3);
        const double* c = q + 2 * ((i + 2) & 3);
        const double z = (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]);
        pos += z > 0;
        neg += z < 0;
    }
    return pos == 4 || neg == 4;
}

// -1 when n entries make a board, else the index of the first entry that breaks a rule (template id outside 0 ..
// OCVAR_MAX_TEMPLATES - 1 or repeated, a corner not finite, the corners not a convex quad of non-zero area); n itself is the
// caller's to check
inline int board_first_bad(const BoardEntry* e, int n) {
    static_assert(OCVAR_MAX_TEMPLATES % 64 == 0, "bit set");
    unsigned long long seen[OCVAR_MAX_TEMPLATES / 64] = {};
    for (int i = 0; i < n; i++) {
        const int t = e[i].templateId;
        if (t < 0 || t >= OCVAR_MAX_TEMPLATES || ((seen[t >> 6] >> (t & 63)) & 1ull)) return i;
        seen[t >> 6] |= 1ull << (t & 63);
        if (!board_quad_ok(e[i].corner)) return i;
    }
    return -1;
}

// ---- phase 1: which records, which corners ----------------------------------------------------------------------------------

// the board index a record may serve (score > 0, a square template of the library, on the board), else -1
OCVAR_HD int board_slot(const MarkerRec& m, const int* map, const TemplateRec* templates, int n_templates) {
    const int t = m.templateId;
    if (!(m.score > 0.0) || t < 0 || t >= n_templates) return -1;
    if (templates[t].width != templates[t].height) return -1;
    return map[t];
}

// the k of code[k] the readout of square sq matches (0..3), -1 for none.  px(x, y): the grey value at (x, y) of the W x H frame.
template <class Px>
OCVAR_HD int board_read_rotation(const Px& px, int W, int H, const float* sq, const TemplateRec& t) {
    const int tw = t.width, th = t.height;
    float m32[9];
    double M[9];
    if (!perspective_from_quad(sq, tw + 2, th + 2, m32))
        for (int i = 0; i < 9; i++) m32[i] = 0.f;
    invert_map(m32, M);
    long long bit = 0;
    for (int i = 0; i < th; i++)
        for (int j = tw - 1; j >= 0; j--) {
            int cx, cy, v = 0;
            if (code_cell(i * tw + j, tw, th, &cx, &cy)) v = warp_sample_px(px, W, H, M, cx + 1, cy + 1) > 100;
            bit = (bit << 1) | v;
        }
    for (int k = 0; k < 4; k++)
        if (bit == t.code[k]) return k;
    return -1;
}

// the observation of board entry b by record m (read rotation k >= 0): board corner c = record corner (c + k) & 3
OCVAR_HD void board_observe(const MarkerRec& m, int b, int k, BoardObs& o) {
    o.index = b;
    for (int c = 0; c < 4; c++) {
        const int r = (c + k) & 3;
        o.sq[2 * c] = m.square[2 * r];
        o.sq[2 * c + 1] = m.square[2 * r + 1];
    }
}

// image area of a quad (seed order)
template <class T>
OCVAR_HD double board_quad_area(const T* q) {
    double s = 0;
    for (int i = 0; i < 4; i++) {
        const int j = (i + 1) & 3;
        s += (double)q[2 * i] * (double)q[2 * j + 1] - (double)q[2 * j] * (double)q[2 * i + 1];
    }
    return fabs(s) * 0.5;
}

// the seeds: indices into the n observations of the up to BOARD_SEEDS largest areas, ties to the lower index
OCVAR_HD int board_pick_seeds(const double* area, int n, int* seed) {
    int ns = 0;
    for (int s = 0; s < BOARD_SEEDS && s < n; s++) {
        int best = -1;
        double ba = -1.0;
        for (int i = 0; i < n; i++) {
            bool taken = false;
            for (int q = 0; q < ns; q++) taken = taken || seed[q] == i;
            if (!taken && area[i] > ba) {
                ba = area[i];
                best = i;
            }
        }
        if (best < 0) break;
        seed[ns++] = best;
    }
    return ns;
}

// ---- phase 2: the solve -----------------------------------------------------------------------------------------------------

// pixel -> undistorted normalised point (cvUndistortPoints: 5 fixed-point iterations when DIST), as square_to_glmatrix_t
template <bool DIST>
OCVAR_HD void board_undistort_t(double u, double v, double fx, double fy, double cx, double cy, const double* dist, double* out) {
    double x = (u - cx) * (1. / fx), y = (v - cy) * (1. / fy);
    if (DIST) {
        const double x0 = x, y0 = y;
        for (int it = 0; it < 5; it++) {
            const double r2 = x * x + y * y;
            const double icd = 1. / (1 + ((dist[4] * r2 + dist[1]) * r2 + dist[0]) * r2);
            const double ddx = 2 * dist[2] * x * y + dist[3] * (r2 + 2 * x * x);
            const double ddy = dist[2] * (r2 + 2 * y * y) + 2 * dist[3] * x * y;
            x = (x0 - ddx) * icd;
            y = (y0 - ddy) * icd;
        }
    }
    out[0] = x;
    out[1] = y;
}

// the projective map of the unit square (0,0) (1,0) (1,1) (0,1) onto quad q (Heckbert), row-major 3x3; false if degenerate
OCVAR_HD bool board_unit_to_quad(const double* q, double* H) {
    const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
    const double dx1 = x1 - x2, dy1 = y1 - y2, dx2 = x3 - x2, dy2 = y3 - y2, sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
    const double den = dx1 * dy2 - dx2 * dy1;
    if (den == 0) return false;
    const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
    H[0] = x1 - x0 + g * x1; H[1] = x3 - x0 + h * x3; H[2] = x0;
    H[3] = y1 - y0 + g * y1; H[4] = y3 - y0 + h * y3; H[5] = y0;
    H[6] = g; H[7] = h; H[8] = 1;
    return true;
}

// The seed of one observation: the homography board quad -> undistorted normalised corners (unit square -> image, after the
// adjugate of unit square -> board), scaled to H[8] = 1, decomposed as square_to_glmatrix_t.  false if degenerate.
template <bool DIST, class T>
OCVAR_HD bool board_seed_t(const BoardObsT<T>& o, const double* board, double fx, double fy, double cx, double cy, const double* dist,
                           double* p) {
    double mn[8], A[9], B[9];
    for (int c = 0; c < 4; c++) board_undistort_t<DIST>((double)o.sq[2 * c], (double)o.sq[2 * c + 1], fx, fy, cx, cy, dist, mn + 2 * c);
    if (!board_unit_to_quad(board, A) || !board_unit_to_quad(mn, B)) return false;
    const double Ai[9] = {A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                          A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                          A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
    double h[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) h[i * 3 + j] = B[i * 3] * Ai[j] + B[i * 3 + 1] * Ai[3 + j] + B[i * 3 + 2] * Ai[6 + j];
    if (h[8] == 0 || !isfinite(h[8])) return false;
    const double is = 1.0 / h[8];
    for (int k = 0; k < 9; k++) h[k] *= is;
    const double n1 = sqrt(h[0] * h[0] + h[3] * h[3] + h[6] * h[6]), n2 = sqrt(h[1] * h[1] + h[4] * h[4] + h[7] * h[7]);
    const double s1 = 1. / fmax(n1, DBL_EPSILON), s2 = 1. / fmax(n2, DBL_EPSILON), s3 = 2. / fmax(n1 + n2, DBL_EPSILON);
    const double a0 = h[0] * s1, a1 = h[3] * s1, a2 = h[6] * s1, b0 = h[1] * s2, b1 = h[4] * s2, b2 = h[7] * s2;
    double Rm[9] = {a0, b0, a1 * b2 - a2 * b1, a1, b1, a2 * b0 - a0 * b2, a2, b2, a0 * b1 - a1 * b0};
    double rv[3];
    rotation_to_rvec(Rm, rv);
    rodrigues_t<false>(rv, Rm, nullptr);
    rotation_to_rvec(Rm, p);
    p[3] = h[2] * s3;
    p[4] = h[5] * s3;
    p[5] = h[8] * s3;
    for (int k = 0; k < 6; k++)
        if (!isfinite(p[k])) return false;
    return true;
}

// reprojection of board point (X, Y, 0) under rotation R (dR: its 3x9 Jacobian when WITH_J) and p: residual e = proj - img,
// Jacobian rows J[0..5] (x) and J[6..11] (y).  The one-point form of pose_core's reproject_t.
template <bool WITH_J, bool DIST>
OCVAR_HD void board_project_t(const double* R, const double* dR, const double* p, double X, double Y, double fx, double fy, double cx,
                              double cy, const double* dist, double u, double v, double* e, double* J) {
    double x = R[0] * X + R[1] * Y + p[3];
    double y = R[3] * X + R[4] * Y + p[4];
    double z = R[6] * X + R[7] * Y + p[5];
    z = z ? 1. / z : 1;
    x *= z;
    y *= z;
    if (!DIST) {
        e[0] = x * fx + cx - u;
        e[1] = y * fy + cy - v;
        if (WITH_J) {
            OCVAR_UNROLL
            for (int j = 0; j < 3; j++) {
                const double* d = dR + 9 * j;
                const double dx0 = X * d[0] + Y * d[1], dy0 = X * d[3] + Y * d[4], dz0 = X * d[6] + Y * d[7];
                J[j] = fx * z * (dx0 - x * dz0);
                J[6 + j] = fy * z * (dy0 - y * dz0);
            }
            J[3] = fx * z; J[4] = 0; J[5] = -fx * x * z;
            J[9] = 0; J[10] = fy * z; J[11] = -fy * y * z;
        }
        return;
    }
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    const double r2 = x * x + y * y;
    const double cd = 1 + (k1 + (k2 + k3 * r2) * r2) * r2;
    const double xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
    const double yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
    e[0] = xd * fx + cx - u;
    e[1] = yd * fy + cy - v;
    if (WITH_J) {
        const double dcd = 2 * (k1 + (2 * k2 + 3 * k3 * r2) * r2);
        const double xdx = cd + x * x * dcd + 2 * p1 * y + 6 * p2 * x, xdy = x * y * dcd + 2 * p1 * x + 2 * p2 * y;
        const double ydx = x * y * dcd + 2 * p1 * x + 2 * p2 * y, ydy = cd + y * y * dcd + 6 * p1 * y + 2 * p2 * x;
        OCVAR_UNROLL
        for (int j = 0; j < 6; j++) {
            double dx, dy;
            if (j < 3) {
                const double* d = dR + 9 * j;
                const double dx0 = X * d[0] + Y * d[1], dy0 = X * d[3] + Y * d[4], dz0 = X * d[6] + Y * d[7];
                dx = z * (dx0 - x * dz0);
                dy = z * (dy0 - y * dz0);
            } else {
                dx = j == 3 ? z : (j == 5 ? -x * z : 0.0);
                dy = j == 4 ? z : (j == 5 ? -y * z : 0.0);
            }
            J[j] = fx * (xdx * dx + xdy * dy);
            J[6 + j] = fy * (ydx * dx + ydy * dy);
        }
    }
}

// Lane `lane`'s partial sums over corners lane, lane + 64, ... of the n observations: BOARD_SUMS values when WITH_J, else e^T e
// alone in s[0].
template <bool WITH_J, bool DIST, class T>
OCVAR_HD void board_partial(const BoardObsT<T>* obs, int n, const BoardEntry* entries, const double* p, double fx, double fy, double cx,
                            double cy, const double* dist, int lane, double* s) {
    double R[9], dR[27];
    rodrigues_t<WITH_J>(p, R, dR);
    OCVAR_UNROLL
    for (int q = 0; q < (WITH_J ? BOARD_SUMS : 1); q++) s[q] = 0.0;
    for (int j = lane; j < 4 * n; j += BOARD_LANES) {
        const BoardObsT<T>& o = obs[j >> 2];
        const int c = j & 3;
        const double* bc = entries[o.index].corner;
        double e[2], J[12];
        board_project_t<WITH_J, DIST>(R, dR, p, bc[2 * c], bc[2 * c + 1], fx, fy, cx, cy, dist, (double)o.sq[2 * c], (double)o.sq[2 * c + 1], e, J);
        if (WITH_J) {
            int k = 0;
            OCVAR_UNROLL
            for (int a = 0; a < 6; a++)
                OCVAR_UNROLL
                for (int b = a; b < 6; b++, k++) s[k] += J[a] * J[b] + J[6 + a] * J[6 + b];
            OCVAR_UNROLL
            for (int a = 0; a < 6; a++) s[21 + a] += J[a] * e[0] + J[6 + a] * e[1];
            s[27] += e[0] * e[0] + e[1] * e[1];
        } else {
            s[0] += e[0] * e[0] + e[1] * e[1];
        }
    }
}

// the fixed combination of the 64 lanes' partial sums (s[lane][BOARD_SUMS], the first nq of each): into s[0]
OCVAR_HD void board_tree(double (*s)[BOARD_SUMS], int nq) {
    for (int half = BOARD_LANES / 2; half >= 1; half >>= 1)
        for (int l = 0; l < half; l++)
            for (int q = 0; q < nq; q++) s[l][q] = s[l][q] + s[l + half][q];
}

// Levenberg-Marquardt from p (in place) as CvLevMarq(6, 4 n corners, 20 iterations | FLT_EPSILON relative step) in
// square_to_glmatrix_t.  sums.jac(p, S): the BOARD_SUMS sums at p; sums.err(p): e^T e at p.  Returns |e| at the final p.
template <class Sums>
OCVAR_HD double board_lm(const Sums& sums, double* p) {
    double prev[6], S[BOARD_SUMS], N[36], Jte[6], dx[6];
    int lambdaLg10 = -3;
    double prevErr = DBL_MAX, errNorm = DBL_MAX;
    for (int iters = 0;;) {
        sums.jac(p, S);
        OCVAR_UNROLL
        for (int i = 0; i < 6; i++) {
            prev[i] = p[i];
            Jte[i] = S[21 + i];
        }
        if (iters == 0) prevErr = sqrt(S[27]);
        for (bool first = true;; first = false) {
            if (!first) {
                errNorm = sqrt(sums.err(p));
                if (!(errNorm > prevErr && ++lambdaLg10 <= 16)) break;
            }
            const double lambda = exp(lambdaLg10 * 2.302585092994046);
            int k = 0;
            OCVAR_UNROLL
            for (int a = 0; a < 6; a++)
                OCVAR_UNROLL
                for (int b = a; b < 6; b++, k++) N[a * 6 + b] = N[b * 6 + a] = S[k];
            OCVAR_UNROLL
            for (int i = 0; i < 6; i++) N[i * 7] *= 1. + lambda;
            if (!chol6(N, Jte, dx))
                OCVAR_UNROLL
                for (int i = 0; i < 6; i++) dx[i] = 0;
            OCVAR_UNROLL
            for (int i = 0; i < 6; i++) p[i] = prev[i] - dx[i];
        }
        lambdaLg10 = lambdaLg10 - 1 > -16 ? lambdaLg10 - 1 : -16;
        double d[6];
        OCVAR_UNROLL
        for (int i = 0; i < 6; i++) d[i] = p[i] - prev[i];
        if (++iters >= 20 || norm_n(d, 6) / norm_n(prev, 6) < FLT_EPSILON) break;
        prevErr = errNorm;
    }
    return errNorm;
}

// The solve of one frame from its n observations (area[i]: board_quad_area of observation i).  Lane-uniform: every lane of the
// device runs it with the same values.
template <bool DIST, class Sums, class T>
OCVAR_HD void board_solve_t(const Sums& sums, const BoardObsT<T>* obs, const double* area, int n, const BoardEntry* entries, double fx,
                            double fy, double cx, double cy, const double* dist, BoardPose& out) {
    for (int k = 0; k < 16; k++) out.glMatrix[k] = 0;
    for (int k = 0; k < 3; k++) out.rvec[k] = out.tvec[k] = 0;
    out.rms = 0;
    out.n_markers = n;
    out.status = 0;
    if (n <= 0) return;
    int seed[BOARD_SEEDS];
    const int ns = board_pick_seeds(area, n, seed);
    double best[6] = {0, 0, 0, 0, 0, 0}, bestErr = DBL_MAX;
    bool found = false;
    for (int s = 0; s < ns; s++) {
        double p[6];
        if (!board_seed_t<DIST>(obs[seed[s]], entries[obs[seed[s]].index].corner, fx, fy, cx, cy, dist, p)) continue;
        const double err = board_lm(sums, p);
        bool finite = isfinite(err);
        for (int k = 0; k < 6; k++) finite = finite && isfinite(p[k]);
        if (!finite || (found && !(err < bestErr))) continue;
        found = true;
        bestErr = err;
        for (int k = 0; k < 6; k++) best[k] = p[k];
    }
    if (!found) {
        out.status = -1;
        return;
    }
    double R[9];
    rodrigues_t<false>(best, R, nullptr);
    gl_from_pose(R, best + 3, out.glMatrix);
    for (int k = 0; k < 3; k++) {
        out.rvec[k] = best[k];
        out.tvec[k] = best[3 + k];
    }
    out.rms = bestErr / sqrt(4.0 * n);
    out.status = 1;
}

// the camera's intrinsics and whether its distortion counts (as square_to_glmatrix)
OCVAR_HD bool board_camera(const CameraRec& cam, double* fx, double* fy, double* cx, double* cy, double* kd) {
    *fx = cam.cameraMatrix[0];
    *fy = cam.cameraMatrix[4];
    *cx = cam.cameraMatrix[2];
    *cy = cam.cameraMatrix[5];
    for (int k = 0; k < 5; k++) kd[k] = cam.distCoeffs[k];
    return kd[0] != 0 || kd[1] != 0 || kd[2] != 0 || kd[3] != 0 || kd[4] != 0;
}

// The host build's sums: all 64 lanes' partials one after the other, then board_tree.
template <bool DIST, class T>
struct BoardSumsHost {
    const BoardObsT<T>* obs;
    int n;
    const BoardEntry* entries;
    double fx, fy, cx, cy;
    const double* dist;
    void jac(const double* p, double* S) const {
        double s[BOARD_LANES][BOARD_SUMS];
        for (int l = 0; l < BOARD_LANES; l++) board_partial<true, DIST>(obs, n, entries, p, fx, fy, cx, cy, dist, l, s[l]);
        board_tree(s, BOARD_SUMS);
        for (int q = 0; q < BOARD_SUMS; q++) S[q] = s[0][q];
    }
    double err(const double* p) const {
        double s[BOARD_LANES][BOARD_SUMS];
        for (int l = 0; l < BOARD_LANES; l++) board_partial<false, DIST>(obs, n, entries, p, fx, fy, cx, cy, dist, l, s[l]);
        board_tree(s, 1);
        return s[0][0];
    }
};

// host: the whole solve of one frame's observations
template <class T>
inline void board_solve_host(const BoardObsT<T>* obs, int n, const BoardEntry* entries, const CameraRec& cam, BoardPose& out) {
    double fx, fy, cx, cy, kd[5], area[BOARD_MAX];
    const bool dist = board_camera(cam, &fx, &fy, &cx, &cy, kd);
    for (int i = 0; i < n && i < BOARD_MAX; i++) area[i] = board_quad_area(obs[i].sq);
    if (dist) board_solve_t<true>(BoardSumsHost<true, T>{obs, n, entries, fx, fy, cx, cy, kd}, obs, area, n, entries, fx, fy, cx, cy, kd, out);
    else board_solve_t<false>(BoardSumsHost<false, T>{obs, n, entries, fx, fy, cx, cy, kd}, obs, area, n, entries, fx, fy, cx, cy, kd, out);
}

}  // namespace ocvar

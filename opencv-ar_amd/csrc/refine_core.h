// refine_core.h -- sub-pixel refinement of a marker's corners on the grey image (opt-in: ocvar_hip_set_corner_refine).
//
// The equations of OpenCV's cornerSubPix.  For a corner c0 and a half window w (pixel centres at integer coordinates):
//   weights  m(i, j) = g(i) g(j), g(k) = (float) exp(-k^2 / w^2), i, j = -w .. w (computed once on the host: refine_args_make)
//   patch    P(i, j) = the grey image at c + (i, j), i, j = -(w+1) .. w+1, bilinear in float, coordinates clamped to the frame
//   sums     over the (2w+1)^2 interior points, gx = P(i+1, j) - P(i-1, j), gy = P(i, j+1) - P(i, j-1), in double:
//            a = S m gx^2, b = S m gx gy, c = S m gy^2, b1 = S m (gx^2 i + gx gy j), b2 = S m (gx gy i + gy^2 j)
//   step     det = a c - b^2; stop if |det| <= DBL_EPSILON^2; else c' = c + (c b1 - b b2, a b2 - b b1) / det, kept in float
//   stop     when c' has left the frame, after max_iter steps, or when |c' - c|^2 <= eps^2
//   result   the final c, or c0 if that is more than w px from c0 in x or in y
// The summation order is part of the definition, so that the host build (tests/emul/refine_emul.cpp) reproduces the device bit
// for bit: REFINE_LANES lanes serve one corner; lane l sums the interior points l, l + 16, l + 32, ... (row-major, x fastest)
// in that order, and the 16 partial sums combine in the tree refine_tree spells out (lane l + lane l ^ 8, then ^ 4, ^ 2, ^ 1:
// the butterfly refine_corners_kernel runs with shuffles gives every lane that same value, since a + b == b + a exactly).
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include <math.h>

namespace ocvar {

constexpr int REFINE_MAX_W = OCVAR_MAX_REFINE_HALF_WIN;
constexpr int REFINE_LANES = 16;   // lanes per corner (one wave: the four corners of one marker)
constexpr double REFINE_DET_MIN = 2.220446049250313e-16 * 2.220446049250313e-16;   // DBL_EPSILON^2

// What a batch's refinement needs, passed by value in the launch arguments (a setting changed while a batch is in flight
// cannot race with it).  half_win 0: off.
struct RefineArgs {
    int half_win;
    int max_iter;
    float eps2;                   // eps^2
    float g[2 * REFINE_MAX_W + 1];   // g[k + w] = (float) exp(-k^2 / w^2)
};

// host only: the arguments of a setting (ranges checked by the caller)
inline RefineArgs refine_args_make(int half_win, int max_iter, float eps) {
    RefineArgs a{};
    a.half_win = half_win;
    a.max_iter = max_iter;
    a.eps2 = eps * eps;
    for (int k = -half_win; k <= half_win && half_win > 0; k++)
        a.g[k + half_win] = (float)exp(-(double)(k * k) / (double)(half_win * half_win));
    return a;
}

// side of the sampled patch, 2w + 3
OCVAR_HD int refine_patch_side(int w) { return 2 * w + 3; }

// Sample the patch around (cx, cy) into P[(2w+3)^2] (row-major, x fastest), the points p = first, first + step, ...
// px(x, y): the grey value at integer (x, y) inside the frame.
template <class Px>
OCVAR_HD void refine_sample(const Px& px, int W, int H, int w, float cx, float cy, float* P, int first, int step) {
    const int side = refine_patch_side(w);
    const float ox = cx - (float)(w + 1), oy = cy - (float)(w + 1);
    float fx = floorf(ox), fy = floorf(oy);
    const float ax = ox - fx, ay = oy - fy;
    // (a corner outside the frame never starts a step; the clamp keeps the integer conversion defined whatever comes in)
    fx = fminf(fmaxf(fx, -64.0f), (float)W);
    fy = fminf(fmaxf(fy, -64.0f), (float)H);
    const int x0 = (int)fx, y0 = (int)fy;
    const float a11 = (1.0f - ax) * (1.0f - ay), a12 = ax * (1.0f - ay), a21 = (1.0f - ax) * ay, a22 = ax * ay;
    for (int p = first; p < side * side; p += step) {
        const int pj = p / side, pi = p - pj * side;
        int xa = x0 + pi, ya = y0 + pj, xb = xa + 1, yb = ya + 1;
        xa = xa < 0 ? 0 : (xa >= W ? W - 1 : xa);
        xb = xb < 0 ? 0 : (xb >= W ? W - 1 : xb);
        ya = ya < 0 ? 0 : (ya >= H ? H - 1 : ya);
        yb = yb < 0 ? 0 : (yb >= H ? H - 1 : yb);
        P[p] = (((float)px(xa, ya) * a11 + (float)px(xb, ya) * a12) + (float)px(xa, yb) * a21) + (float)px(xb, yb) * a22;
    }
}

// Lane `lane`'s partial sums s = (a, b, c, b1, b2) over the interior points lane, lane + 16, ...
OCVAR_HD void refine_partial(const float* P, const float* g, int w, int lane, double* s) {
    const int n = 2 * w + 1, side = n + 2;
    for (int q = 0; q < 5; q++) s[q] = 0.0;
    for (int k = lane; k < n * n; k += REFINE_LANES) {
        const int jj = k / n, ii = k - jj * n;   // 0 .. 2w
        const float* c = P + (jj + 1) * side + (ii + 1);
        const float gx = c[1] - c[-1], gy = c[side] - c[-side];
        const double m = (double)(g[ii] * g[jj]);
        const double i = (double)(ii - w), j = (double)(jj - w);
        const double gxx = (double)gx * (double)gx * m, gxy = (double)gx * (double)gy * m, gyy = (double)gy * (double)gy * m;
        s[0] += gxx;
        s[1] += gxy;
        s[2] += gyy;
        s[3] += gxx * i + gxy * j;
        s[4] += gxy * i + gyy * j;
    }
}

// the fixed combination of the 16 lanes' partial sums (s[lane][5]): into s[0]
OCVAR_HD void refine_tree(double (*s)[5]) {
    for (int half = REFINE_LANES / 2; half >= 1; half >>= 1)
        for (int l = 0; l < half; l++)
            for (int q = 0; q < 5; q++) s[l][q] = s[l][q] + s[l + half][q];
}

// One step from the five sums: moves (cx, cy) unless det is too small; true when the corner stops here (det, left the frame,
// converged).  The caller counts the steps.
OCVAR_HD bool refine_update(const double* s, float& cx, float& cy, int W, int H, float eps2) {
    const double det = s[0] * s[2] - s[1] * s[1];
    if (fabs(det) <= REFINE_DET_MIN) return true;
    const double dx = (s[2] * s[3] - s[1] * s[4]) / det, dy = (s[0] * s[4] - s[1] * s[3]) / det;
    const float nx = (float)((double)cx + dx), ny = (float)((double)cy + dy);
    const float ex = nx - cx, ey = ny - cy;
    const float err = ex * ex + ey * ey;
    cx = nx;
    cy = ny;
    if (cx < 0.0f || cx >= (float)W || cy < 0.0f || cy >= (float)H) return true;
    return err <= eps2;
}

// the final rule: a corner that moved more than w px from where it started (in x or in y) keeps its start
OCVAR_HD void refine_finish(float x0, float y0, int w, float& cx, float& cy) {
    if (fabsf(cx - x0) > (float)w || fabsf(cy - y0) > (float)w) {
        cx = x0;
        cy = y0;
    }
}

// The whole refinement of one corner in one thread (the host build): P is scratch of (2w+3)^2 floats.
template <class Px>
OCVAR_HD void refine_corner(const Px& px, int W, int H, const RefineArgs& ra, float* P, float& cx, float& cy) {
    const int w = ra.half_win;
    if (w <= 0) return;
    const float x0 = cx, y0 = cy;
    for (int iter = 0; iter < ra.max_iter;) {
        refine_sample(px, W, H, w, cx, cy, P, 0, 1);
        double s[REFINE_LANES][5];
        for (int l = 0; l < REFINE_LANES; l++) refine_partial(P, ra.g, w, l, s[l]);
        refine_tree(s);
        const bool stop = refine_update(s[0], cx, cy, W, H, ra.eps2);
        iter++;
        if (stop) break;
    }
    refine_finish(x0, y0, w, cx, cy);
}

}  // namespace ocvar

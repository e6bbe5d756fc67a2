// flow_core.h -- marker records carried from one frame to the next by sparse pyramidal Lucas-Kanade on their four corners
// (opt-in: ocvar_hip_flow_records).  The equations of OpenCV's calcOpticalFlowPyrLK, with these choices: central differences
// in place of Scharr, float bilinear sampling (refine_core.h's) in place of 14-bit fixed point, the smallest-eigenvalue test
// written without a square root, no oscillation rule.  What cvarCompareSquare's "four points from optical flow"
// (opencvar.cpp:323-367) were meant to come from.
//
// Pyramid of a W x H frame (integers only):
//   level 0   the library's grey of the frame: the byte of OCVAR_FMT_GRAY, else (1868 B + 9617 G + 4899 R + 8192) >> 14 (hd.h)
//   level l+1 W' = (W_l + 1) >> 1, H' = (H_l + 1) >> 1; pixel (x, y) = (sum + 128) >> 8, sum = S_{i,j=-2..2} k_i k_j
//             P_l(r(2x + i, W_l), r(2y + j, H_l)), k = 1 4 6 4 1, r(t, n) = -t for t < 0, 2n - 2 - t for t >= n, else t
//             (OpenCV's pyrDown on 8-bit images, BORDER_REFLECT_101)
//   levels    0 .. L, L the largest l <= levels with min(W_l, H_l) >= 2w + 3 (w: the half window); level 0 is always used
// One corner, from p (float32) in frame A to frame B:
//   start     0 <= x <= W-1 and 0 <= y <= H-1 (a NaN fails the comparisons), else code -1
//   levels    l = L .. 0 with p_l = p * 2^-l and the guess g, (0, 0) at level L:
//     template  I = the (2w+3)^2 patch of A's level l around p_l (refine_sample: bilinear in float, coordinates clamped)
//     gradients on the (2w+1)^2 interior Ix = 0.5f * (I(i+1, j) - I(i-1, j)), Iy alike
//     sums      a = S Ix^2, b = S Ix Iy, c = S Iy^2 in double
//     texture   with n = (2w+1)^2, T = min_eig n: a - T >= 0, c - T >= 0, (a - T)(c - T) - b^2 >= 0 and |a c - b^2| >
//               DBL_EPSILON^2; without it the level contributes d = 0, and at level 0 the corner fails with code -2
//     steps     d = (0, 0); each step: J = the patch of B's level l around (p_l + g) + d, e1 = S (I - J) Ix, e2 = S (I - J) Iy
//               in double, s = (c e1 - b e2, a e2 - b e1) / (a c - b^2), d' = (float) (d + s).  If (p_l + g) + d' has left
//               [0, W_l - 1] x [0, H_l - 1] the level stops and keeps d -- at level 0 the corner fails with code -3.  Else
//               d = d', and the level stops when |s|^2 <= eps^2 or after max_iter steps.
//     hand-down g_{l-1} = 2 (g_l + d_l) in float
//   result    q = (p + g_0) + d_0 in float
//   error     err = (float) (S |I - J| / n) at level 0 with J sampled once more around q; with max_err > 0, err > max_err
//             fails with code -4
//   back      with fb_max > 0 the same tracker (error limit included) runs from q in B back to A; a failed back track or a
//             squared distance to p above fb_max^2 (in double) fails with code -5
// The summation order is part of the definition (refine_core.h's): FLOW_LANES lanes serve a corner, lane l sums the interior
// points l, l + 16, ... (row-major, x fastest) in that order and the 16 partial sums combine in flow_tree's order -- what the
// butterfly of flow_track_kernel leaves in every lane.
// One record: its corners are tracked independently; the status is the code of the lowest-numbered failing corner, else -6 if
// the tracked quad is not strictly convex (overlay_core.h's predicate), else 1.  Status 1: the output is the input with the
// square replaced and, with OCVAR_FLOW_POSE, glMatrix solved from it (square_to_glmatrix with the camera of the call and the
// record's aspectRatio).  Any other status: the record is copied unchanged.  A corner's error is -1.0f when it was not reached.
//
// Only + - * / and comparisons in float and double, floorf and integers (-ffp-contract=off) -- glMatrix apart, which is
// pose_core.h's: the host build (tests/emul/flow_emul.cpp) gives the bytes of the kernels (flow.hip).  flow_pyramid_level,
// flow_track_corner and flow_track_frame are that host reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "overlay_core.h"
#include "pose_core.h"
#include "refine_core.h"
#include "tail_core.h"

namespace ocvar {

constexpr int FLOW_MAX_W = OCVAR_MAX_FLOW_HALF_WIN;
constexpr int FLOW_MAX_LEVELS = OCVAR_MAX_FLOW_LEVELS;
constexpr int FLOW_LANES = REFINE_LANES;
constexpr int FLOW_FLAGS = OCVAR_FLOW_POSE;
constexpr int FLOW_MAX_SIDE = 2 * FLOW_MAX_W + 3;

// The parameters of a call as the kernels take them, by value in the launch arguments.
struct FlowArgs {
    int half_win, levels, max_iter, flags;
    float eps2;       // eps^2
    float min_eig, max_err, fb_max;
};

// host only (ranges checked by the caller)
inline FlowArgs flow_args_make(const OcvarFlowParams& p) {
    return FlowArgs{p.half_win, p.levels, p.max_iter, p.flags, p.eps * p.eps, p.min_eig, p.max_err, p.fb_max};
}

// Where the levels of one frame's pyramid lie in the workspace (the layout is no part of the definition): level l is w[l] x h[l]
// bytes, rows pitch[l] (w[l] rounded up to whole 64-byte sectors) apart, off[l] bytes after the pyramid's first byte.
struct FlowGeom {
    int L;   // the levels used are 0 .. L
    int w[FLOW_MAX_LEVELS + 1], h[FLOW_MAX_LEVELS + 1], pitch[FLOW_MAX_LEVELS + 1];
    long long off[FLOW_MAX_LEVELS + 1];
    long long bytes;   // of all FLOW_MAX_LEVELS + 1 levels, a multiple of 256
};

OCVAR_HD FlowGeom flow_geom(int W, int H, int half_win, int levels) {
    FlowGeom g;
    g.L = 0;
    long long off = 0;
    int w = W, h = H;
    for (int l = 0; l <= FLOW_MAX_LEVELS; l++) {
        g.w[l] = w;
        g.h[l] = h;
        g.pitch[l] = (w + 63) & ~63;
        g.off[l] = off;
        off += (long long)g.pitch[l] * h;
        if (l >= 1 && l <= levels && g.L == l - 1 && (w < h ? w : h) >= 2 * half_win + 3) g.L = l;
        w = (w + 1) >> 1;
        h = (h + 1) >> 1;
    }
    g.bytes = (off + 255) & ~255LL;
    return g;
}

// the grey of the pixel at p in format fmt
OCVAR_HD int flow_grey(const uint8_t* p, int fmt) {
    if (fmt == OCVAR_FMT_GRAY) return p[0];
    const bool bgr = fmt == OCVAR_FMT_BGR || fmt == OCVAR_FMT_BGRA;
    const int B = bgr ? p[0] : p[2], G = p[1], R = bgr ? p[2] : p[0];
    return (1868 * B + 9617 * G + 4899 * R + 8192) >> 14;
}

OCVAR_HD int flow_reflect(int t, int n) {
    t = t < 0 ? -t : (t >= n ? 2 * n - 2 - t : t);
    return t < 0 ? 0 : (t >= n ? n - 1 : t);   // (sides below 3 only: no level the tracker uses)
}
OCVAR_HD int flow_k(int i) { return (i == 0 || i == 4) ? 1 : (i == 2 ? 6 : 4); }

// Pixel (x, y) of the level above a W x H level whose pixels px(x, y) gives.
template <class Px>
OCVAR_HD int flow_down_px(const Px& px, int W, int H, int x, int y) {
    int sum = 0;
    for (int j = 0; j < 5; j++) {
        const int yy = flow_reflect(2 * y + j - 2, H);
        int row = 0;
        for (int i = 0; i < 5; i++) row += flow_k(i) * px(flow_reflect(2 * x + i - 2, W), yy);
        sum += flow_k(j) * row;
    }
    return (sum + 128) >> 8;
}

OCVAR_HD bool flow_inside(float x, float y, int W, int H) { return x >= 0.0f && x <= (float)(W - 1) && y >= 0.0f && y <= (float)(H - 1); }

// Lane `lane`'s partial sums over the interior points lane, lane + 16, ...: (a, b, c) of the template I
OCVAR_HD void flow_grad_partial(const float* I, int w, int lane, double* s) {
    const int n = 2 * w + 1, side = n + 2;
    s[0] = s[1] = s[2] = 0.0;
    for (int k = lane; k < n * n; k += FLOW_LANES) {
        const int jj = k / n, ii = k - jj * n;
        const float* c = I + (jj + 1) * side + (ii + 1);
        const float ix = 0.5f * (c[1] - c[-1]), iy = 0.5f * (c[side] - c[-side]);
        s[0] += (double)ix * (double)ix;
        s[1] += (double)ix * (double)iy;
        s[2] += (double)iy * (double)iy;
    }
}

// (e1, e2) of the template I against the patch J
OCVAR_HD void flow_diff_partial(const float* I, const float* J, int w, int lane, double* s) {
    const int n = 2 * w + 1, side = n + 2;
    s[0] = s[1] = 0.0;
    for (int k = lane; k < n * n; k += FLOW_LANES) {
        const int jj = k / n, ii = k - jj * n, at = (jj + 1) * side + (ii + 1);
        const float* c = I + at;
        const float ix = 0.5f * (c[1] - c[-1]), iy = 0.5f * (c[side] - c[-side]);
        const double dt = (double)(c[0] - J[at]);
        s[0] += dt * (double)ix;
        s[1] += dt * (double)iy;
    }
}

// S |I - J|
OCVAR_HD void flow_abs_partial(const float* I, const float* J, int w, int lane, double* s) {
    const int n = 2 * w + 1, side = n + 2;
    s[0] = 0.0;
    for (int k = lane; k < n * n; k += FLOW_LANES) {
        const int jj = k / n, ii = k - jj * n, at = (jj + 1) * side + (ii + 1);
        const float dt = I[at] - J[at];
        s[0] += (double)(dt < 0.0f ? -dt : dt);
    }
}

// the fixed combination of the 16 lanes' partial sums (refine_tree's order): into s[0]
template <int Q>
OCVAR_HD void flow_tree(double (*s)[Q]) {
    for (int half = FLOW_LANES / 2; half >= 1; half >>= 1)
        for (int l = 0; l < half; l++)
            for (int q = 0; q < Q; q++) s[l][q] = s[l][q] + s[l + half][q];
}

// the texture test on g = (a, b, c)
OCVAR_HD bool flow_texture(const double* g, int w, float min_eig) {
    const double n = (double)((2 * w + 1) * (2 * w + 1)), T = (double)min_eig * n;
    const double a = g[0] - T, c = g[2] - T, det = g[0] * g[2] - g[1] * g[1];
    return a >= 0.0 && c >= 0.0 && a * c - g[1] * g[1] >= 0.0 && (det < 0.0 ? -det : det) > REFINE_DET_MIN;
}

// One step at level `level` (W x H) from g = (a, b, c) and e = (e1, e2), the patch J having been sampled around (bx, by) + d:
// moves d unless the new position has left the level (code -3 at level 0); true when the level stops here.  The caller counts.
OCVAR_HD bool flow_step(const double* g, const double* e, float bx, float by, int W, int H, int level, float eps2, float& dx, float& dy,
                        int& code) {
    const double det = g[0] * g[2] - g[1] * g[1];
    const double sx = (g[2] * e[0] - g[1] * e[1]) / det, sy = (g[0] * e[1] - g[1] * e[0]) / det;
    const float nx = (float)((double)dx + sx), ny = (float)((double)dy + sy);
    if (!flow_inside(bx + nx, by + ny, W, H)) {
        if (level == 0) code = -3;
        return true;
    }
    dx = nx;
    dy = ny;
    return sx * sx + sy * sy <= (double)eps2;
}

OCVAR_HD float flow_err(double sum_abs, int w) { return (float)(sum_abs / (double)((2 * w + 1) * (2 * w + 1))); }

// the forward-backward rule: `back` and (bx, by) are the back track's code and result, (px, py) the corner it should return to
OCVAR_HD int flow_fb_code(int back, float bx, float by, float px, float py, float fb_max) {
    if (back != 1) return -5;
    const double ex = (double)bx - (double)px, ey = (double)by - (double)py;
    return ex * ex + ey * ey > (double)fb_max * (double)fb_max ? -5 : 1;
}

// the record's status from its corners' codes and the tracked quad
OCVAR_HD int flow_record_status(const int* codes, const float* sq) {
    for (int i = 0; i < 4; i++)
        if (codes[i] != 1) return codes[i];
    return quad_strictly_convex(sq) ? 1 : -6;
}

// the pixels of level l of the pyramid at `pyr`
struct FlowLevelPx {
    const uint8_t* p;
    int pitch;
    OCVAR_HD int operator()(int x, int y) const { return p[(long long)y * pitch + x]; }
};
OCVAR_HD FlowLevelPx flow_level_px(const uint8_t* pyr, const FlowGeom& g, int l) { return FlowLevelPx{pyr + g.off[l], g.pitch[l]}; }

// ---- the host reference (one thread) ------------------------------------------------------------------------------------------

// Level 0 of a frame in format fmt: dst rows dst_pitch bytes apart.
inline void flow_grey_level(const uint8_t* frame, int W, int H, long long row_stride, int fmt, uint8_t* dst, int dst_pitch) {
    const int bpp = overlay_bpp(fmt);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) dst[(long long)y * dst_pitch + x] = (uint8_t)flow_grey(frame + (long long)y * row_stride + (long long)x * bpp, fmt);
}

// The level above the W x H level src: ((W + 1) >> 1) x ((H + 1) >> 1) pixels into dst.
inline void flow_pyramid_level(const uint8_t* src, int W, int H, int src_pitch, uint8_t* dst, int dst_pitch) {
    const FlowLevelPx px{src, src_pitch};
    for (int y = 0; y < (H + 1) >> 1; y++)
        for (int x = 0; x < (W + 1) >> 1; x++) dst[(long long)y * dst_pitch + x] = (uint8_t)flow_down_px(px, W, H, x, y);
}

// Levels 0 .. g.L of a frame into the g.bytes bytes at pyr.
inline void flow_build_pyramid(const uint8_t* frame, long long row_stride, int fmt, const FlowGeom& g, uint8_t* pyr) {
    flow_grey_level(frame, g.w[0], g.h[0], row_stride, fmt, pyr, g.pitch[0]);
    for (int l = 0; l < g.L; l++) flow_pyramid_level(pyr + g.off[l], g.w[l], g.h[l], g.pitch[l], pyr + g.off[l + 1], g.pitch[l + 1]);
}

// One corner from (px, py) in pyramid A to pyramid B, without the back track: the code (1, -1 .. -4), the result (the start when
// the corner fails) and the error (-1.0f when it was not reached).  I, J: scratch of (2w+3)^2 floats each.
inline int flow_track_forward(const uint8_t* A, const uint8_t* B, const FlowGeom& g, const FlowArgs& fa, float px, float py, float* I,
                              float* J, float* qx, float* qy, float* err) {
    const int w = fa.half_win;
    *qx = px;
    *qy = py;
    *err = -1.0f;
    if (!flow_inside(px, py, g.w[0], g.h[0])) return -1;
    float gx = 0.0f, gy = 0.0f, dx = 0.0f, dy = 0.0f;
    for (int l = g.L; l >= 0; l--) {
        const float sc = 1.0f / (float)(1 << l);
        const float bx = px * sc + gx, by = py * sc + gy;
        refine_sample(flow_level_px(A, g, l), g.w[l], g.h[l], w, px * sc, py * sc, I, 0, 1);
        double s[FLOW_LANES][3];
        for (int k = 0; k < FLOW_LANES; k++) flow_grad_partial(I, w, k, s[k]);
        flow_tree<3>(s);
        dx = dy = 0.0f;
        if (!flow_texture(s[0], w, fa.min_eig)) {
            if (l == 0) return -2;
        } else {
            int code = 1;
            for (int iter = 0; iter < fa.max_iter; iter++) {
                refine_sample(flow_level_px(B, g, l), g.w[l], g.h[l], w, bx + dx, by + dy, J, 0, 1);
                double e[FLOW_LANES][2];
                for (int k = 0; k < FLOW_LANES; k++) flow_diff_partial(I, J, w, k, e[k]);
                flow_tree<2>(e);
                if (flow_step(s[0], e[0], bx, by, g.w[l], g.h[l], l, fa.eps2, dx, dy, code)) break;
            }
            if (code != 1) return code;
        }
        if (l > 0) {
            gx = 2.0f * (gx + dx);
            gy = 2.0f * (gy + dy);
        }
    }
    *qx = (px + gx) + dx;
    *qy = (py + gy) + dy;
    refine_sample(flow_level_px(B, g, 0), g.w[0], g.h[0], w, *qx, *qy, J, 0, 1);   // (I is level 0's template)
    double a[FLOW_LANES][1];
    for (int k = 0; k < FLOW_LANES; k++) flow_abs_partial(I, J, w, k, a[k]);
    flow_tree<1>(a);
    *err = flow_err(a[0][0], w);
    if (fa.max_err > 0.0f && *err > fa.max_err) return -4;
    return 1;
}

// One corner with the forward-backward check: the code (1, -1 .. -5).
inline int flow_track_corner(const uint8_t* A, const uint8_t* B, const FlowGeom& g, const FlowArgs& fa, float px, float py, float* I, float* J,
                             float* qx, float* qy, float* err) {
    int code = flow_track_forward(A, B, g, fa, px, py, I, J, qx, qy, err);
    if (code == 1 && fa.fb_max > 0.0f) {
        float bx, by, berr;
        const int back = flow_track_forward(B, A, g, fa, *qx, *qy, I, J, &bx, &by, &berr);
        code = flow_fb_code(back, bx, by, px, py, fa.fb_max);
    }
    return code;
}

// One frame pair: the record slots k < min(count, slots) of `in` from pyramid A to pyramid B into `out` (which may be `in`),
// status [slots] and err [slots][4] (either may be nullptr).  Slots at or beyond the count get status 0 and nothing else.
// Returns the number of records tracked.
inline int flow_track_frame(const uint8_t* A, const uint8_t* B, const FlowGeom& g, const FlowArgs& fa, const CameraRec& cam, const MarkerRec* in,
                            int count, int slots, MarkerRec* out, int* status, float* err) {
    static thread_local float I[FLOW_MAX_SIDE * FLOW_MAX_SIDE], J[FLOW_MAX_SIDE * FLOW_MAX_SIDE];
    const int n = count < slots ? count : slots;
    int tracked = 0;
    for (int k = 0; k < slots; k++) {
        if (k >= n) {
            if (status) status[k] = 0;
            continue;
        }
        MarkerRec r = in[k];
        int codes[4];
        float sq[8];
        for (int c = 0; c < 4; c++) {
            float e;
            codes[c] = flow_track_corner(A, B, g, fa, r.square[2 * c], r.square[2 * c + 1], I, J, sq + 2 * c, sq + 2 * c + 1, &e);
            if (err) err[4 * k + c] = e;
        }
        const int st = flow_record_status(codes, sq);
        if (st == 1) {
            tracked++;
            for (int q = 0; q < 8; q++) r.square[q] = sq[q];
            if (fa.flags & OCVAR_FLOW_POSE) square_to_glmatrix(r.square, cam, r.aspectRatio, r.glMatrix);
        }
        out[k] = r;
        if (status) status[k] = st;
    }
    return tracked;
}

}  // namespace ocvar

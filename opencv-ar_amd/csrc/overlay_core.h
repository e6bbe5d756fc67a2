// overlay_core.h -- drawing a per-template overlay image onto every marker a frame's records hold (opt-in:
// ocvar_hip_set_overlay / ocvar_hip_render / ocvar_hip_render_records).  What the reference's caller does with its records
// (samples/ARTest.cpp draws on every marker it finds), for frames that stay in device memory; no GL.
//
// An overlay is a straight-alpha RGBA8 image of ow x oh texels (2 .. OCVAR_MAX_OVERLAY_SIDE each way).  For one record:
//   map      m32 = perspective_from_quad(record.square, ow, oh): frame pixels -> texel coordinates, record corners 0..3 to
//            (0,0) (ow-1,0) (ow-1,oh-1) (0,oh-1).  No map, a corner that is not finite, corners that are not a strictly convex
//            quad (three in a line, two equal, a bow-tie: what perspective_from_quad's two zero tests catch only in part;
//            the detector's quads are convex), score <= 0, or no overlay for the record's template and no default overlay:
//            the record draws nothing.
//   box      the record is drawn inside the bounding box of its four corners, grown on every side by 1 + (its longer side) / 16
//            px and clipped to the frame.  (The growth holds the 1/64-texel slack of the coverage rule below for any overlay
//            under any sane perspective; the box is what bounds the work.)
//   pixel    for integer (x, y), in double from the float32 m32: w = m6 x + m7 y + m8 (w == 0: not drawn), u = (m0 x + m1 y +
//            m2) / w, U = (int) rint(clamp(32 u)) with warp_sample_px's clamp, V likewise.  Covered iff 0 <= U <= 32 (ow-1) and
//            0 <= V <= 32 (oh-1) -- no sign test on w: the preimage of the rectangle under a projective map is the quad.
//   sample   ix = U >> 5, fx = U & 31 (y alike); texels (ix, iy), (min(ix+1, ow-1), iy) and the same pair one row down (row
//            clamped alike); every one of R, G, B, A is (sum p_k w_k + 512) >> 10 with the weights (32-fx)(32-fy), fx (32-fy),
//            (32-fx) fy, fx fy.  Plain bilinear: no mipmaps (an overlay far larger than its marker aliases) and no
//            anti-aliasing of the quad's edge.
//   blend    a == 0: the pixel is not touched.  Else per colour channel out = (c a + d (255 - a) + 127) / 255 on the frame's
//            value d.  BGR / BGRA take B, G, R; RGB / RGBA take R, G, B; byte 3 of a four-channel pixel is never written;
//            OCVAR_FMT_GRAY blends the library's grey of the colour, (1868 B + 9617 G + 4899 R + 8192) >> 14 (hd.h), into its byte.
// A frame is composited record by record in output order, k = 0 .. min(count, stride) - 1: a later record is blended over
// what the earlier ones left.  The order is part of the definition.
//
// Which way up: texel (0, 0) -- the first of the image's bytes, its top-left -- lands on record corner 0, the top-right texel on
// corner 1, bottom-right on 2, bottom-left on 3.  For a marker decoded at orient 1, 2 or 4 the record's corners 0..3 are the
// template image's bottom-left, bottom-right, top-right and top-left corners, whichever way the marker is turned in the frame
// (rot_square has brought them there; templates are loaded flipped vertically, see ocvar_hip_set_board): the overlay lies on
// the marker as the printed pattern does, its top row along the template image's bottom row.  A marker decoded at orient 3 --
// seen turned by 180 degrees against orient 1 -- keeps the corner order it was found with, as in the reference (only orient 2
// and 4 rotate the corners, opencvar.cpp:753-760), so its record, its glMatrix and its overlay are turned by 180 degrees on it.
//
// All arithmetic is integer or IEEE double (-ffp-contract=off): the host build (tests/emul/overlay_emul.cpp) gives the bytes
// of the kernels (overlay.hip).  overlay_render_frame is that host reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "decode_core.h"
#include "tail_core.h"
#include <math.h>

namespace ocvar {

constexpr int OVL_MAX = OCVAR_MAX_OVERLAYS;
constexpr int OVL_MAX_SIDE = OCVAR_MAX_OVERLAY_SIDE;

// One overlay image: w x h texels, tightly packed, texel = R | G << 8 | B << 16 | A << 24 (the bytes R G B A in memory).
struct OverlayTex {
    const uint32_t* px;   // nullptr: the slot is free
    int w, h;
};

// A context's overlays (device memory on the device, host memory in the host build).
struct OverlayTable {
    OverlayTex tex[OVL_MAX];
    int dflt;                          // slot of the default overlay, -1: none
    int map[OCVAR_MAX_TEMPLATES];      // templateId -> slot, -1: none of its own
};

// What the draw kernel needs of one record: the map and the overlay; its box travels beside it (OverlayBox).
struct OverlayDraw {
    float m[9];
    int slot;
    int pad[2];
};   // 48 bytes
struct OverlayBox { int x0, y0, x1, y1; };   // inclusive; x0 > x1: the record draws nothing
static_assert(sizeof(OverlayDraw) == 48 && sizeof(OverlayBox) == 16, "overlay workspace records");

// bytes per pixel of a frame format, 0: unknown
OCVAR_HD int overlay_bpp(int fmt) {
    return (fmt == OCVAR_FMT_BGR || fmt == OCVAR_FMT_RGB) ? 3 : ((fmt == OCVAR_FMT_BGRA || fmt == OCVAR_FMT_RGBA) ? 4 : (fmt == OCVAR_FMT_GRAY ? 1 : 0));
}

// Strictly convex: the four turns of the quad sq (8 floats) have one strict sign.  (flow_core.h asks the same of a tracked quad.)
OCVAR_HD bool quad_strictly_convex(const float* sq) {
    int pos = 0, neg = 0;
    for (int i = 0; i < 4; i++) {
        const float* p = sq + 2 * i;
        const float* q = sq + 2 * ((i + 1) & 3);
        const float* s = sq + 2 * ((i + 2) & 3);
        const double z = ((double)q[0] - p[0]) * ((double)s[1] - q[1]) - ((double)q[1] - p[1]) * ((double)s[0] - q[0]);
        pos += z > 0.0;
        neg += z < 0.0;
    }
    return pos == 4 || neg == 4;
}

// One record of a W x H frame: its map, overlay and box; false (and an empty box): it draws nothing.
OCVAR_HD bool overlay_setup(const MarkerRec& r, const OverlayTable& tab, int W, int H, OverlayDraw& d, OverlayBox& b) {
    b.x0 = 1; b.y0 = 1; b.x1 = 0; b.y1 = 0;
    d.slot = -1;
    d.pad[0] = d.pad[1] = 0;
    for (int i = 0; i < 9; i++) d.m[i] = 0.f;
    if (!(r.score > 0.0)) return false;
    const int t = r.templateId;
    int slot = (t >= 0 && t < OCVAR_MAX_TEMPLATES) ? tab.map[t] : -1;
    if (slot < 0) slot = tab.dflt;
    if (slot < 0 || slot >= OVL_MAX) return false;
    double minx = r.square[0], maxx = minx, miny = r.square[1], maxy = miny;
    for (int i = 0; i < 4; i++) {
        const double x = r.square[2 * i], y = r.square[2 * i + 1];
        if (!isfinite(x) || !isfinite(y)) return false;
        minx = x < minx ? x : minx;
        maxx = x > maxx ? x : maxx;
        miny = y < miny ? y : miny;
        maxy = y > maxy ? y : maxy;
    }
    if (!quad_strictly_convex(r.square)) return false;
    const OverlayTex tex = tab.tex[slot];
    if (!perspective_from_quad(r.square, tex.w, tex.h, d.m)) return false;
    const double side = (maxx - minx) > (maxy - miny) ? (maxx - minx) : (maxy - miny);
    const double g = 1.0 + side / 16.0;
    const double lx = floor(minx - g), ly = floor(miny - g), hx = ceil(maxx + g), hy = ceil(maxy + g);
    if (!(hx >= 0.0) || !(hy >= 0.0) || !(lx <= (double)(W - 1)) || !(ly <= (double)(H - 1))) return false;   // (wholly outside)
    b.x0 = lx > 0.0 ? (int)lx : 0;
    b.y0 = ly > 0.0 ? (int)ly : 0;
    b.x1 = hx < (double)(W - 1) ? (int)hx : W - 1;
    b.y1 = hy < (double)(H - 1) ? (int)hy : H - 1;
    d.slot = slot;
    return true;
}

// Frame pixel (x, y) under map m: its texel coordinates in 1/32 texel; false: not covered by the ow x oh overlay.
OCVAR_HD bool overlay_coords(const float* m, int x, int y, int ow, int oh, int* U, int* V) {
    const double dx = (double)x, dy = (double)y;
    const double w = (double)m[6] * dx + (double)m[7] * dy + (double)m[8];
    if (w == 0.0) return false;
    const double u = ((double)m[0] * dx + (double)m[1] * dy + (double)m[2]) / w;
    const double v = ((double)m[3] * dx + (double)m[4] * dy + (double)m[5]) / w;
    const double fu = fmax(-2147483648.0, fmin(2147483647.0, 32.0 * u));
    const double fv = fmax(-2147483648.0, fmin(2147483647.0, 32.0 * v));
    const int iu = (int)rint(fu), iv = (int)rint(fv);
    *U = iu;
    *V = iv;
    return iu >= 0 && iu <= 32 * (ow - 1) && iv >= 0 && iv <= 32 * (oh - 1);
}

// The overlay's colour at (U, V) / 32, 0 <= U <= 32 (w-1), 0 <= V <= 32 (h-1): R | G << 8 | B << 16 | A << 24.
OCVAR_HD unsigned overlay_sample(const OverlayTex& t, int U, int V) {
    const int ix = U >> 5, iy = V >> 5, fx = U & 31, fy = V & 31;
    const int ix1 = ix + 1 < t.w ? ix + 1 : t.w - 1, iy1 = iy + 1 < t.h ? iy + 1 : t.h - 1;
    const uint32_t* r0 = t.px + (size_t)iy * t.w;
    const uint32_t* r1 = t.px + (size_t)iy1 * t.w;
    const unsigned p00 = r0[ix], p01 = r0[ix1], p10 = r1[ix], p11 = r1[ix1];
    const unsigned w00 = (unsigned)((32 - fx) * (32 - fy)), w01 = (unsigned)(fx * (32 - fy)), w10 = (unsigned)((32 - fx) * fy),
                   w11 = (unsigned)(fx * fy);
    unsigned out = 0;
    OCVAR_UNROLL
    for (int c = 0; c < 4; c++) {
        const int s = 8 * c;
        const unsigned v = (((p00 >> s) & 255u) * w00 + ((p01 >> s) & 255u) * w01 + ((p10 >> s) & 255u) * w10 + ((p11 >> s) & 255u) * w11 + 512u) >> 10;
        out |= v << s;
    }
    return out;
}

OCVAR_HD unsigned overlay_blend(unsigned c, unsigned a, unsigned d) { return (c * a + d * (255u - a) + 127u) / 255u; }

// The colour bytes of a frame pixel in format fmt under colour rgba (alpha > 0): d[0 .. 2] (d[0] alone in OCVAR_FMT_GRAY) in
// memory order, blended in place.
OCVAR_HD void overlay_blend_px(int fmt, unsigned rgba, unsigned* d) {
    const unsigned R = rgba & 255u, G = (rgba >> 8) & 255u, B = (rgba >> 16) & 255u, a = rgba >> 24;
    if (fmt == OCVAR_FMT_GRAY) {
        d[0] = overlay_blend((1868u * B + 9617u * G + 4899u * R + 8192u) >> 14, a, d[0]);
    } else {
        const bool bgr = fmt == OCVAR_FMT_BGR || fmt == OCVAR_FMT_BGRA;
        d[0] = overlay_blend(bgr ? B : R, a, d[0]);
        d[1] = overlay_blend(G, a, d[1]);
        d[2] = overlay_blend(bgr ? R : B, a, d[2]);
    }
}

// The host reference: one W x H frame in format fmt (rows row_stride bytes apart) under its records recs[0 .. min(count,
// stride) - 1], sequentially.  Returns the number of records that drew (had a map, an overlay and a box in the frame).
inline int overlay_render_frame(uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* recs, int count, int stride,
                                const OverlayTable& tab) {
    const int bpp = overlay_bpp(fmt), nc = bpp == 1 ? 1 : 3;
    int n = count < stride ? count : stride, drawn = 0;
    for (int k = 0; k < n; k++) {
        OverlayDraw d;
        OverlayBox b;
        if (!overlay_setup(recs[k], tab, W, H, d, b)) continue;
        drawn++;
        const OverlayTex tex = tab.tex[d.slot];
        for (int y = b.y0; y <= b.y1; y++)
            for (int x = b.x0; x <= b.x1; x++) {
                int U, V;
                if (!overlay_coords(d.m, x, y, tex.w, tex.h, &U, &V)) continue;
                const unsigned rgba = overlay_sample(tex, U, V);
                if ((rgba >> 24) == 0u) continue;
                uint8_t* p = frame + (long long)y * row_stride + (long long)x * bpp;
                unsigned v[3] = {p[0], nc > 1 ? p[1] : 0u, nc > 1 ? p[2] : 0u};
                overlay_blend_px(fmt, rgba, v);
                for (int c = 0; c < nc; c++) p[c] = (uint8_t)v[c];
            }
    }
    return drawn;
}

}  // namespace ocvar

// annotate_core.h -- stroking what a marker record holds into its frame (opt-in: ocvar_hip_annotate /
// ocvar_hip_annotate_records): the outline of its square, a dot on corner 0, a cube and the axes of its pose, its template id.
// What a caller draws first when setting up a camera or a board (ArUco's drawDetectedMarkers / drawFrameAxes; the reference's
// sample draws a cube on every square, samples/ARTest.cpp), for frames that stay in device memory.  This is the library's own
// stroke rule: parity with OpenCV's line rasteriser is neither claimed nor tested.
//
// The style (OcvarAnnotateStyle, by value with every call) names the primitives (flags), the stroke width `thickness` (1 .. 16
// px), axis_length and cube_height in the marker model's units, five straight-alpha R G B A colours and label_scale.
//
// One record, in this fixed order (primitive index p):
//   0..3    OUTLINE  the edges of `square`, corner k to corner (k + 1) & 3.  Colour: `outline`; with COLOR_BY_TEMPLATE
//                    ANNO_PALETTE[templateId mod 12] with the outline's alpha; `unmatched` for a record with score <= 0.
//   4       CORNER0  a zero-length segment at corner 0, stroked with width 2 thickness + 1: a disc of that diameter.
//   5..16   CUBE     base edges (corner k to k + 1 of the model rectangle), top edges, then the four uprights.  The base is the
//                    marker rectangle (-r,-1,0) (r,-1,0) (r,1,0) (-r,1,0), r = the record's aspectRatio (pose_core.h's model);
//                    the top is the same rectangle at z = cube_height, the side the pose's Z axis points to.
//   17..19  AXES     from the model origin to (L,0,0), (0,L,0), (0,0,L), L = axis_length: red, green, blue with the outline's alpha.
//   20      LABEL    templateId (>= 0) in decimal, from the 5 x 7 font ANNO_FONT: n digits, cells of s x s px, glyphs 6 cells
//                    apart: (6 n - 1) s px wide and 7 s high, axis-aligned.  Its left column is ox = rint(cx - (width - 1) / 2),
//                    cx = (x0 + x1 + x2 + x3) / 4 in double, its top row oy likewise from the height: centred on the mean of the
//                    corners.  s = label_scale, or with label_scale 0 the largest s in 1 .. 8 with (24 s)^2 <= the squared length
//                    of the quad's shortest edge (1 if there is none): four digits fit across a square marker.
// Which records draw: k < min(count, stride); all eight corner coordinates finite; score > 0 -- or, with UNMATCHED, score <= 0,
// and then OUTLINE and CORNER0 only.  CUBE and AXES also need sixteen finite glMatrix values.  No convexity requirement: the
// outline of a bow-tie is its four edges.
//
// Pose: (R, t) inverts gl_from_pose: R[r][c] = s_r s_c glMatrix[4 c + r] with s = (-1, -1, 1), t = (m[12], m[13], -m[14]).  A model
// point X goes to Xc = R X + t; z <= 0 drops the segment it ends; else x = Xc.x (1 / z), y = Xc.y (1 / z), then reproject_t's lens
// model (k1 k2 p1 p2 k3; skipped when all five are zero), u = xd fx + cx, v = yd fy + cy with the camera passed by value.  Only
// end points are projected; strokes are straight between them.  A projection that is not finite drops the segment.
//
// Stroke: end points are rounded once, in setup, to 1/16 px: a = (int) rint(clamp(16 u)), the clamp to +-16 ANNO_MAX_COORD
// (ANNO_MAX_COORD = 2^20 px; a far end point moves there, coordinate by coordinate, as overlay_coords clamps its texel
// coordinates).  With frames of at most 32767 px a side every difference below is under 2^25 in magnitude: every product and sum
// of two products fits int64 and is below 2^53, exact as a double.  Pixel (x, y) has P = (16 x, 16 y); with d = B - A, v = P - A,
// R2 = (8 w)^2 for stroke width w:
//     dot = v.d    dot <= 0: covered iff v.v <= R2         dot >= d.d: covered iff (P - B).(P - B) <= R2
//     else covered iff (double) cross * (double) cross <= (double) R2 * (double) (d.d),  cross = v.x d.y - v.y d.x
// (the only rounding steps are those two double products, one fixed sequence).  A primitive is tested inside its box: the
// bounding box of its end points grown by the stroke radius, floor((min - 8 w) / 16) .. ceil((max + 8 w) / 16), clipped to the
// frame -- every covered pixel of the frame lies in it; a primitive with an empty box, and a record all of whose boxes are empty,
// draws nothing.  The label covers (x, y) iff 0 <= x - ox < width, 0 <= y - oy < height, column (x - ox) / s = 6 g + c with
// c < 5, and bit 4 - c of row (y - oy) / s of digit g's glyph is set.
//
// Compositing: within a record a pixel takes the colour of the LAST primitive in the order above that covers it, and that
// colour is blended once with overlay_blend_px (alpha 0: untouched; byte 3 of a four-channel pixel never written; GRAY takes the
// library's grey of the colour) -- joints and crossings of half-transparent strokes do not darken twice.  Records composite in
// output order, later over earlier.  Pixels outside the frame are not drawn.
//
// All arithmetic is integer or IEEE double (-ffp-contract=off): the host build (tests/emul/annotate_emul.cpp) gives the bytes of
// the kernels (annotate.hip).  annotate_frame is that host reference, sequential.  The workspace holds, per marker record slot,
// one AnnoRec (680 bytes) and one AnnoBox (16 bytes): OCVAR_ANNO_RECORD_BYTES = 696.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "overlay_core.h"
#include "pose_core.h"
#include "tail_core.h"
#include <math.h>

namespace ocvar {

constexpr int ANNO_DRAW_FLAGS = OCVAR_ANNO_OUTLINE | OCVAR_ANNO_CORNER0 | OCVAR_ANNO_AXES | OCVAR_ANNO_CUBE | OCVAR_ANNO_LABEL;
constexpr int ANNO_FLAGS = ANNO_DRAW_FLAGS | OCVAR_ANNO_UNMATCHED | OCVAR_ANNO_COLOR_BY_TEMPLATE;
constexpr int ANNO_MAX_COORD = OCVAR_ANNO_MAX_COORD;   // px
constexpr int ANNO_SEGS = 20, ANNO_SEG_DOT = 4, ANNO_SEG_CUBE = 5, ANNO_SEG_AXES = 17;
constexpr int ANNO_MAX_DIGITS = 10;   // of a non-negative int

// One stroke: end points in 1/16 px, the box it is tested in (inclusive; x0 > x1: dropped), its colour R | G << 8 | B << 16 | A << 24
// and its radius 8 width in 1/16 px.
struct AnnoSeg {
    int ax, ay, bx, by;
    short x0, y0, x1, y1;
    unsigned rgba;
    int r;
};   // 32 bytes
// What the draw kernel needs of one record; its overall box travels beside it (AnnoBox).
struct AnnoRec {
    AnnoSeg seg[ANNO_SEGS];
    int ox, oy;                 // the label's left column and top row
    int scale, n;               // cell size in px; digits (0: no label)
    unsigned char digit[12];    // most significant first
    unsigned rgba;
    short x0, y0, x1, y1;       // the label's box (inclusive; x0 > x1: dropped)
};   // 680 bytes
struct AnnoBox {
    short x0, y0, x1, y1;   // inclusive, clipped to the frame; x0 > x1: the record draws nothing
    unsigned live;          // bit p: primitive p has a box (bit ANNO_SEGS: the label)
    unsigned pad;
};
OCVAR_HD void anno_box_grow(AnnoBox& b, int x0, int y0, int x1, int y1) {
    if (b.x0 > b.x1) {
        b.x0 = (short)x0; b.y0 = (short)y0; b.x1 = (short)x1; b.y1 = (short)y1;
    } else {
        b.x0 = (short)(x0 < b.x0 ? x0 : b.x0);
        b.y0 = (short)(y0 < b.y0 ? y0 : b.y0);
        b.x1 = (short)(x1 > b.x1 ? x1 : b.x1);
        b.y1 = (short)(y1 > b.y1 ? y1 : b.y1);
    }
}
static_assert(sizeof(AnnoSeg) == 32 && sizeof(AnnoRec) == 680 && sizeof(AnnoBox) == 16, "annotate workspace records");
static_assert(sizeof(AnnoRec) + sizeof(AnnoBox) == OCVAR_ANNO_RECORD_BYTES, "bytes per record slot");
static_assert(sizeof(OcvarAnnotateStyle) == 56, "OcvarAnnotateStyle layout");

// The 5 x 7 font: digit d, row r (0: top) in bits 5 r .. 5 r + 4, bit 4 of a row its left column.
//   0: 01110 10001 10011 10101 11001 10001 01110    1: 00100 01100 00100 00100 00100 00100 01110
//   2: 01110 10001 00001 00010 00100 01000 11111    3: 11111 00010 00100 00010 00001 10001 01110
//   4: 00010 00110 01010 10010 11111 00010 00010    5: 11111 10000 11110 00001 00001 10001 01110
//   6: 00110 01000 10000 11110 10001 10001 01110    7: 11111 00001 00010 00100 01000 01000 01000
//   8: 01110 10001 10001 01110 10001 10001 01110    9: 01110 10001 10001 01111 00001 00010 01100
#define ANNO_GLYPH(a, b, c, d, e, f, g)                                                                                      \
    ((unsigned long long)(a) | (unsigned long long)(b) << 5 | (unsigned long long)(c) << 10 | (unsigned long long)(d) << 15 | \
     (unsigned long long)(e) << 20 | (unsigned long long)(f) << 25 | (unsigned long long)(g) << 30)
OCVAR_HD unsigned long long anno_glyph(int d) {
    const unsigned long long ANNO_FONT[10] = {
        ANNO_GLYPH(0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), ANNO_GLYPH(0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
        ANNO_GLYPH(0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F), ANNO_GLYPH(0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),
        ANNO_GLYPH(0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), ANNO_GLYPH(0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
        ANNO_GLYPH(0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), ANNO_GLYPH(0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
        ANNO_GLYPH(0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E), ANNO_GLYPH(0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C)};
    return ANNO_FONT[d];
}
#undef ANNO_GLYPH

// The palette of COLOR_BY_TEMPLATE: R | G << 8 | B << 16 (alpha comes from the outline colour).
OCVAR_HD unsigned anno_palette(int t) {
    const unsigned ANNO_PALETTE[12] = {0x0000E6u /* red */,   0x00B400u /* green */,  0xE66400u /* blue */,   0x00D2FFu /* yellow */,
                                       0xE600E6u /* magenta */, 0xE6E600u /* cyan */, 0x0082FFu /* orange */, 0xC83C96u /* purple */,
                                       0x32C8AAu /* lime */,   0x9678FFu /* pink */,   0x828200u /* teal */,   0x285AAAu /* brown */};
    const int i = ((t % 12) + 12) % 12;
    return ANNO_PALETTE[i];
}

OCVAR_HD unsigned anno_rgba(const uint8_t* c) { return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 | (unsigned)c[3] << 24; }

// What the entry points refuse of a style (a camera is asked for by AXES and CUBE): 0 = accepted, else which rule.
inline int anno_style_bad(const OcvarAnnotateStyle* s, bool have_camera) {
    if (!s) return 1;
    if (s->thickness < 1 || s->thickness > OCVAR_ANNO_MAX_THICKNESS) return 2;
    if (s->label_scale < 0 || s->label_scale > OCVAR_ANNO_MAX_LABEL_SCALE) return 3;
    if (!isfinite(s->axis_length) || !isfinite(s->cube_height) || s->axis_length < 0.0 || s->cube_height < 0.0) return 4;
    if (s->flags & ~ANNO_FLAGS) return 5;
    if (!(s->flags & ANNO_DRAW_FLAGS)) return 6;
    if ((s->flags & (OCVAR_ANNO_AXES | OCVAR_ANNO_CUBE)) && !have_camera) return 7;
    return 0;
}

inline void anno_default_style(OcvarAnnotateStyle* s) {
    *s = OcvarAnnotateStyle{};
    s->flags = OCVAR_ANNO_OUTLINE | OCVAR_ANNO_CORNER0 | OCVAR_ANNO_LABEL;
    s->thickness = 2;
    s->label_scale = 0;
    s->axis_length = 1.0;
    s->cube_height = 1.0;
    const uint8_t outline[4] = {0, 255, 0, 255}, unmatched[4] = {160, 160, 160, 255}, corner0[4] = {255, 0, 0, 255},
                  cube[4] = {0, 255, 255, 255}, label[4] = {255, 255, 0, 255};
    for (int i = 0; i < 4; i++) {
        s->outline[i] = outline[i];
        s->unmatched[i] = unmatched[i];
        s->corner0[i] = corner0[i];
        s->cube[i] = cube[i];
        s->label[i] = label[i];
    }
}

// A coordinate in px -> 1/16 px, rounded once and clamped; false: not finite.
OCVAR_HD bool anno_fix(double u, int* out) {
    if (!isfinite(u)) return false;
    const double lim = 16.0 * (double)ANNO_MAX_COORD;
    *out = (int)rint(fmax(-lim, fmin(lim, 16.0 * u)));
    return true;
}

OCVAR_HD int anno_floor16(int v) { return v >> 4; }              // floor(v / 16)
OCVAR_HD int anno_ceil16(int v) { return (v + 15) >> 4; }        // ceil(v / 16)

OCVAR_HD void anno_seg_drop(AnnoSeg& s) {
    s.ax = s.ay = s.bx = s.by = 0;
    s.x0 = 1; s.y0 = 1; s.x1 = 0; s.y1 = 0;
    s.rgba = 0;
    s.r = 0;
}

// The stroke of width w px from (ax, ay) to (bx, by) (1/16 px) in a W x H frame; its box grows the record's box b.
OCVAR_HD void anno_seg_make(AnnoSeg& s, int ax, int ay, int bx, int by, int w, unsigned rgba, int W, int H, AnnoBox& b) {
    const int r = 8 * w;
    int x0 = anno_floor16((ax < bx ? ax : bx) - r), x1 = anno_ceil16((ax > bx ? ax : bx) + r);
    int y0 = anno_floor16((ay < by ? ay : by) - r), y1 = anno_ceil16((ay > by ? ay : by) + r);
    x0 = x0 > 0 ? x0 : 0;
    y0 = y0 > 0 ? y0 : 0;
    x1 = x1 < W - 1 ? x1 : W - 1;
    y1 = y1 < H - 1 ? y1 : H - 1;
    if (x0 > x1 || y0 > y1) {
        anno_seg_drop(s);
        return;
    }
    s.ax = ax; s.ay = ay; s.bx = bx; s.by = by;
    s.x0 = (short)x0; s.y0 = (short)y0; s.x1 = (short)x1; s.y1 = (short)y1;
    s.rgba = rgba;
    s.r = r;
    anno_box_grow(b, x0, y0, x1, y1);
}

// Model point (X, Y, Z) under (R, t) and the camera -> 1/16 px; false: behind the camera or not finite.
OCVAR_HD bool anno_project(const double* R, const double* t, const CameraRec& cam, bool dist, double X, double Y, double Z, int* u, int* v) {
    double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    const double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z;
    x *= iz;
    y *= iz;
    const double fx = cam.cameraMatrix[0], fy = cam.cameraMatrix[4], cx = cam.cameraMatrix[2], cy = cam.cameraMatrix[5];
    if (dist) {
        const double k1 = cam.distCoeffs[0], k2 = cam.distCoeffs[1], p1 = cam.distCoeffs[2], p2 = cam.distCoeffs[3], k3 = cam.distCoeffs[4];
        const double r2 = x * x + y * y;
        const double cd = 1 + (k1 + (k2 + k3 * r2) * r2) * r2;
        const double xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = xd;
        y = yd;
    }
    return anno_fix(x * fx + cx, u) && anno_fix(y * fy + cy, v);
}

// One record of a W x H frame under style st and camera cam: its primitives and its box; false (and an empty box): it draws
// nothing.
OCVAR_HD void anno_box_empty(AnnoBox& b) {
    b.x0 = 1; b.y0 = 1; b.x1 = 0; b.y1 = 0;
    b.live = 0;
    b.pad = 0;
}

OCVAR_HD bool anno_setup(const MarkerRec& r, const OcvarAnnotateStyle& st, const CameraRec& cam, int W, int H, AnnoRec& a, AnnoBox& b) {
    anno_box_empty(b);
    for (int p = 0; p < ANNO_SEGS; p++) anno_seg_drop(a.seg[p]);
    a.ox = a.oy = 0;
    a.scale = 1;
    a.n = 0;
    for (int i = 0; i < 12; i++) a.digit[i] = 0;
    a.rgba = 0;
    a.x0 = 1; a.y0 = 1; a.x1 = 0; a.y1 = 0;
    const bool matched = r.score > 0.0;
    if (!matched && !((st.flags & OCVAR_ANNO_UNMATCHED) && r.score <= 0.0)) return false;
    int cx[4], cy[4];
    for (int i = 0; i < 4; i++)
        if (!anno_fix((double)r.square[2 * i], &cx[i]) || !anno_fix((double)r.square[2 * i + 1], &cy[i])) return false;
    const int w = st.thickness;
    const unsigned oa = (unsigned)st.outline[3] << 24;
    if (st.flags & OCVAR_ANNO_OUTLINE) {
        const unsigned c = !matched ? anno_rgba(st.unmatched) : ((st.flags & OCVAR_ANNO_COLOR_BY_TEMPLATE) ? (anno_palette(r.templateId) | oa) : anno_rgba(st.outline));
        for (int i = 0; i < 4; i++) anno_seg_make(a.seg[i], cx[i], cy[i], cx[(i + 1) & 3], cy[(i + 1) & 3], w, c, W, H, b);
    }
    if (st.flags & OCVAR_ANNO_CORNER0) anno_seg_make(a.seg[ANNO_SEG_DOT], cx[0], cy[0], cx[0], cy[0], 2 * w + 1, anno_rgba(st.corner0), W, H, b);
    if (matched && (st.flags & (OCVAR_ANNO_CUBE | OCVAR_ANNO_AXES))) {
        bool fin = true;
        for (int q = 0; q < 16; q++) fin = fin && isfinite(r.glMatrix[q]);
        if (fin) {
            const double sg[3] = {-1.0, -1.0, 1.0};
            double R[9], t[3] = {r.glMatrix[12], r.glMatrix[13], -r.glMatrix[14]};
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[3 * i + j] = sg[i] * sg[j] * r.glMatrix[4 * j + i];
            const double* kd = cam.distCoeffs;
            const bool dist = kd[0] != 0 || kd[1] != 0 || kd[2] != 0 || kd[3] != 0 || kd[4] != 0;
            if (st.flags & OCVAR_ANNO_CUBE) {
                const double ra = r.aspectRatio, MX[4] = {-ra, ra, ra, -ra}, MY[4] = {-1, -1, 1, 1};
                int u[8], v[8];
                bool ok[8];
                for (int i = 0; i < 8; i++) ok[i] = anno_project(R, t, cam, dist, MX[i & 3], MY[i & 3], i < 4 ? 0.0 : st.cube_height, &u[i], &v[i]);
                const unsigned c = anno_rgba(st.cube);
                for (int e = 0; e < 12; e++) {
                    const int i0 = e < 4 ? e : (e < 8 ? e : e - 8), i1 = e < 4 ? ((e + 1) & 3) : (e < 8 ? 4 + ((e + 1) & 3) : e - 4);
                    if (ok[i0] && ok[i1]) anno_seg_make(a.seg[ANNO_SEG_CUBE + e], u[i0], v[i0], u[i1], v[i1], w, c, W, H, b);
                }
            }
            if (st.flags & OCVAR_ANNO_AXES) {
                int u0, v0;
                if (anno_project(R, t, cam, dist, 0.0, 0.0, 0.0, &u0, &v0)) {
                    const double L = st.axis_length;
                    for (int i = 0; i < 3; i++) {
                        int u1, v1;
                        if (anno_project(R, t, cam, dist, i == 0 ? L : 0.0, i == 1 ? L : 0.0, i == 2 ? L : 0.0, &u1, &v1))
                            anno_seg_make(a.seg[ANNO_SEG_AXES + i], u0, v0, u1, v1, w, (255u << (8 * i)) | oa, W, H, b);
                    }
                }
            }
        }
    }
    if (matched && (st.flags & OCVAR_ANNO_LABEL) && r.templateId >= 0) {
        int s = st.label_scale;
        if (s == 0) {
            double m2 = 0.0;
            for (int i = 0; i < 4; i++) {
                const double dx = (double)r.square[2 * ((i + 1) & 3)] - (double)r.square[2 * i];
                const double dy = (double)r.square[2 * ((i + 1) & 3) + 1] - (double)r.square[2 * i + 1];
                const double l2 = dx * dx + dy * dy;
                m2 = (i == 0 || l2 < m2) ? l2 : m2;
            }
            s = 1;
            for (int k = 2; k <= OCVAR_ANNO_MAX_LABEL_SCALE; k++)
                if ((double)(24 * k) * (double)(24 * k) <= m2) s = k;
        }
        int n = 0, v = r.templateId;
        unsigned char rev[ANNO_MAX_DIGITS];
        do {
            rev[n++] = (unsigned char)(v % 10);
            v /= 10;
        } while (v > 0);
        const int lw = (6 * n - 1) * s, lh = 7 * s;
        const double mx = ((double)r.square[0] + (double)r.square[2] + (double)r.square[4] + (double)r.square[6]) * 0.25;
        const double my = ((double)r.square[1] + (double)r.square[3] + (double)r.square[5] + (double)r.square[7]) * 0.25;
        const double lim = (double)ANNO_MAX_COORD;
        const int ox = (int)rint(fmax(-lim, fmin(lim, mx - 0.5 * (double)(lw - 1))));
        const int oy = (int)rint(fmax(-lim, fmin(lim, my - 0.5 * (double)(lh - 1))));
        const int x0 = ox > 0 ? ox : 0, y0 = oy > 0 ? oy : 0;
        const int x1 = ox + lw - 1 < W - 1 ? ox + lw - 1 : W - 1, y1 = oy + lh - 1 < H - 1 ? oy + lh - 1 : H - 1;
        if (x0 <= x1 && y0 <= y1) {
            a.ox = ox; a.oy = oy;
            a.scale = s;
            a.n = n;
            for (int i = 0; i < n; i++) a.digit[i] = rev[n - 1 - i];
            a.rgba = anno_rgba(st.label);
            a.x0 = (short)x0; a.y0 = (short)y0; a.x1 = (short)x1; a.y1 = (short)y1;
            anno_box_grow(b, x0, y0, x1, y1);
            b.live |= 1u << ANNO_SEGS;
        }
    }
    for (int p = 0; p < ANNO_SEGS; p++)
        if (a.seg[p].x0 <= a.seg[p].x1) b.live |= 1u << p;
    return b.x0 <= b.x1;
}

// Is the centre of pixel (x, y) within the stroke?  (One fixed sequence; see the opening comment for the ranges.)
OCVAR_HD bool anno_seg_covers(const AnnoSeg& s, int x, int y) {
    const int px = 16 * x, py = 16 * y;
    const int dx = s.bx - s.ax, dy = s.by - s.ay, vx = px - s.ax, vy = py - s.ay;
    const long long dot = (long long)vx * dx + (long long)vy * dy;
    const long long r2 = (long long)s.r * s.r;
    if (dot <= 0) return (long long)vx * vx + (long long)vy * vy <= r2;
    const long long dd = (long long)dx * dx + (long long)dy * dy;
    if (dot >= dd) {
        const int wx = px - s.bx, wy = py - s.by;
        return (long long)wx * wx + (long long)wy * wy <= r2;
    }
    const long long cross = (long long)vx * dy - (long long)vy * dx;
    const double c = (double)cross;
    return c * c <= (double)r2 * (double)dd;
}

// Does the record's label cover pixel (x, y) of its box?
OCVAR_HD bool anno_label_covers(const AnnoRec& a, int x, int y) {
    const int col = (x - a.ox) / a.scale, row = (y - a.oy) / a.scale;   // (inside the box both differences are >= 0)
    const int g = col / 6, c = col - 6 * g;
    if (c >= 5 || g >= a.n || row >= 7) return false;
    return (anno_glyph(a.digit[g]) >> (5 * row + 4 - c)) & 1ull;
}

// The colour record a gives pixel (x, y): that of the last primitive that covers it; false: none does.
OCVAR_HD bool anno_colour(const AnnoRec& a, int x, int y, unsigned* rgba) {
    bool hit = false;
    for (int p = 0; p < ANNO_SEGS; p++) {
        const AnnoSeg& s = a.seg[p];
        if (x < s.x0 || x > s.x1 || y < s.y0 || y > s.y1) continue;
        if (anno_seg_covers(s, x, y)) {
            *rgba = s.rgba;
            hit = true;
        }
    }
    if (a.n > 0 && x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1 && anno_label_covers(a, x, y)) {
        *rgba = a.rgba;
        hit = true;
    }
    return hit;
}

// The host reference: one W x H frame in format fmt (rows row_stride bytes apart) under its records recs[0 .. min(count, stride)
// - 1], sequentially.  Returns the number of records that drew (had a primitive with a box in the frame).
inline int annotate_frame(uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* recs, int count, int stride,
                          const OcvarAnnotateStyle& st, const CameraRec& cam) {
    const int bpp = overlay_bpp(fmt), nc = bpp == 1 ? 1 : 3;
    int n = count < stride ? count : stride, drawn = 0;
    for (int k = 0; k < n; k++) {
        AnnoRec a;
        AnnoBox b;
        if (!anno_setup(recs[k], st, cam, W, H, a, b)) continue;
        drawn++;
        for (int y = b.y0; y <= b.y1; y++)
            for (int x = b.x0; x <= b.x1; x++) {
                unsigned rgba = 0;
                if (!anno_colour(a, x, y, &rgba) || (rgba >> 24) == 0u) continue;
                uint8_t* p = frame + (long long)y * row_stride + (long long)x * bpp;
                unsigned v[3] = {p[0], nc > 1 ? p[1] : 0u, nc > 1 ? p[2] : 0u};
                overlay_blend_px(fmt, rgba, v);
                for (int c = 0; c < nc; c++) p[c] = (uint8_t)v[c];
            }
    }
    return drawn;
}

}  // namespace ocvar

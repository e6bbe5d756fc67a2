// levels_core.h -- the grey levels of device-resident frames stretched, for the whole frame or per tile with the maps of
// neighbouring tiles blended (opt-in: ocvar_hip_levels).  The detection path has two fixed photometric thresholds from the reference,
// the adaptive threshold's constant 8 (opencvar.cpp:181) and the cut at grey 100 on the warped patch before the code grid is read
// (:724): an under-exposed stream whose white cells lie below 100, or a washed-out one whose black cells lie above it, yields
// squares but no marker.  This step brings such frames back without a trip through the host.  It is the library's own rule: there
// is no OpenCV function to be in parity with; with low_ppm = high_ppm = 0 and no gain cap reached it is normalize(..., NORM_MINMAX)
// up to rounding.  All arithmetic is integer.
//
//   input    n_frames frames of W x H pixels in any OCVAR_FMT_*; g is the library's grey of a pixel, (1868 B + 9617 G + 4899 R +
//            8192) >> 14 with the format's channel order (yuv_core.h: yuv_grey; what grey_of and flow_grey compute), the byte itself
//            for GRAY.
//   output   one GRAY plane per frame.  Detected with ocvar_hip_set_input_format(GRAY) its records are in the source frame's own
//            coordinates: nothing is carried across, and drawing goes onto the original frames.
//   params   OcvarLevelsParams { tiles_x, tiles_y, low_ppm, high_ppm, max_gain_q8 }: tiles 1 .. 16 per axis, tiles_x tiles_y <= 64,
//            tiles_x <= W, tiles_y <= H (defaults 1, 1); low_ppm, high_ppm 0 .. 500000 (10000, 10000: 1 % clipped at each end);
//            max_gain_q8 256 .. 65280 (2048: a gain of at most 8).
//   tiles    edges xe[i] = (i W) / tiles_x, ye[j] = (j H) / tiles_y (floor); tile (j, i) owns xe[i] <= x < xe[i+1], ye[j] <= y <
//            ye[j+1]; its histogram is the 256 counts of g over those n pixels.
//   LUT      k_lo = (n low_ppm) / 1000000, k_hi = (n high_ppm) / 1000000 in 64 bits; lo the smallest v with #{g <= v} > k_lo, hi
//            the largest v with #{g >= v} > k_hi; minr = (255 * 256 + max_gain_q8 - 1) / max_gain_q8; if hi - lo < minr (which
//            covers lo > hi): lo = min(max((lo + hi - minr) >> 1, 0), 255 - minr) with an arithmetic shift, hi = lo + minr.
//            lut[v] = min(max((v - lo) 510 + (hi - lo), 0) / (2 (hi - lo)), 255): (v - lo) 255 / (hi - lo) rounded to nearest.
//   blend    between tile centres.  Along x for pixel x: c2[i] = xe[i] + xe[i+1], p = 2 x + 1, i0 the largest i with c2[i] <= p
//            clamped to 0 .. max(tiles_x - 2, 0), i1 = min(i0 + 1, tiles_x - 1), wx = i1 > i0 ? clamp(((p - c2[i0]) 256) /
//            (c2[i1] - c2[i0]), 0, 256) : 0; along y the same with ye: j0, j1, wy.  top = lut[j0][i0][g] (256 - wx) + lut[j0][i1][g]
//            wx, bot the same on row j1, out = (top (256 - wy) + bot wy + 32768) >> 16.  With one tile the result is lut[g].
//
// The plan the kernels (levels.hip) and the host build share: a tile's rows are cut into slabs of LEVELS_SLAB_ROWS for the
// histogram; the pixels whose i0 is k form cell k of an axis, [k ? c2[k] >> 1 : 0, k < cells - 1 ? c2[k+1] >> 1 : extent), and a
// cell is cut into segments of at most LEVELS_SEG_W pixels along x and LEVELS_SEG_H along y, each of which one workgroup of the
// apply kernel covers (levels_segment).  The host build (tests/emul/levels_emul.cpp) gives the kernels' bytes; levels_frames is
// that host reference, sequential.
#pragma once
#include "hd.h"
#include "ocvar_hip.h"
#include "patch_core.h"
#include "yuv_core.h"

namespace ocvar {

constexpr int LEVELS_MAX_SIDE = 32767;
constexpr int LEVELS_MAX_TILES_AXIS = 16, LEVELS_MAX_TILES = 64;
constexpr int LEVELS_MAX_PPM = 500000, LEVELS_MIN_GAIN_Q8 = 256, LEVELS_MAX_GAIN_Q8 = 65280;
constexpr int LEVELS_WS_FRAMES = 256;        // frames of one round through the workspace
constexpr int LEVELS_SLAB_ROWS = 32;         // rows of a tile one workgroup of the histogram kernel counts
constexpr int LEVELS_SEG_W = 256, LEVELS_SEG_H = 32;   // the apply kernel's rectangle
constexpr long long LEVELS_HIST_BYTES = 1024, LEVELS_LUT_BYTES = 256;
// the workspace: [LEVELS_WS_FRAMES][LEVELS_MAX_TILES] histograms of 256 counts, then as many LUTs of 256 bytes
constexpr long long LEVELS_WS_LUT_OFFSET = (long long)LEVELS_WS_FRAMES * LEVELS_MAX_TILES * LEVELS_HIST_BYTES;
constexpr long long LEVELS_WS_BYTES = LEVELS_WS_LUT_OFFSET + (long long)LEVELS_WS_FRAMES * LEVELS_MAX_TILES * LEVELS_LUT_BYTES;

inline void levels_default_params(OcvarLevelsParams* p) {
    p->tiles_x = p->tiles_y = 1;
    p->low_ppm = p->high_ppm = 10000;
    p->max_gain_q8 = 2048;
}

// 0, or which rule p breaks on W x H frames: 1 the tiles, 2 the fractions, 3 the gain cap
OCVAR_HD int levels_params_bad(const OcvarLevelsParams& p, int W, int H) {
    if (p.tiles_x < 1 || p.tiles_x > LEVELS_MAX_TILES_AXIS || p.tiles_y < 1 || p.tiles_y > LEVELS_MAX_TILES_AXIS ||
        p.tiles_x * p.tiles_y > LEVELS_MAX_TILES || p.tiles_x > W || p.tiles_y > H)
        return 1;
    if (p.low_ppm < 0 || p.low_ppm > LEVELS_MAX_PPM || p.high_ppm < 0 || p.high_ppm > LEVELS_MAX_PPM) return 2;
    if (p.max_gain_q8 < LEVELS_MIN_GAIN_Q8 || p.max_gain_q8 > LEVELS_MAX_GAIN_Q8) return 3;
    return 0;
}

// the grey of the pixel whose first three bytes are c0 c1 c2 (GRAY: c0 alone)
OCVAR_HD int levels_grey(int c0, int c1, int c2, int fmt) {
    if (fmt == OCVAR_FMT_GRAY) return c0;
    const bool bgr = fmt == OCVAR_FMT_BGR || fmt == OCVAR_FMT_BGRA;
    return yuv_grey(bgr ? c0 : c2, c1, bgr ? c2 : c0);
}

// edge i of `tiles` tiles over `extent` pixels
OCVAR_HD int levels_edge(int i, int extent, int tiles) { return (i * extent) / tiles; }
// twice the centre of tile i
OCVAR_HD int levels_c2(int i, int extent, int tiles) { return levels_edge(i, extent, tiles) + levels_edge(i + 1, extent, tiles); }
// cells of an axis, and the first pixel of cell k (k = cells: the extent)
OCVAR_HD int levels_cells(int tiles) { return tiles > 1 ? tiles - 1 : 1; }
OCVAR_HD int levels_cell_start(int k, int extent, int tiles) {
    return k <= 0 ? 0 : (k >= levels_cells(tiles) ? extent : levels_c2(k, extent, tiles) >> 1);
}

// The blend of pixel x along one axis: the two tiles and the weight of the second, 0 .. 256.
OCVAR_HD void levels_axis(int x, int extent, int tiles, int* i0, int* i1, int* w) {
    const int p = 2 * x + 1;
    int k = 0;
    for (int i = 1; i + 1 < tiles; i++)      // c2 ascends: the largest i <= tiles - 2 with c2[i] <= p
        if (levels_c2(i, extent, tiles) <= p) k = i;
    const int k1 = k + 1 < tiles ? k + 1 : tiles - 1;
    int wt = 0;
    if (k1 > k) {
        const int a = levels_c2(k, extent, tiles), b = levels_c2(k1, extent, tiles);
        wt = p <= a ? 0 : ((p - a) * 256) / (b - a);
        wt = wt > 256 ? 256 : wt;
    }
    *i0 = k, *i1 = k1, *w = wt;
}

// The weight alone, for a pixel known to lie in cell k (what levels_axis gives it): from twice the two centres of the cell, a = b = 0
// with one tile on the axis.
OCVAR_HD void levels_cell_centres(int k, int extent, int tiles, int* a, int* b) {
    *a = tiles < 2 ? 0 : levels_c2(k, extent, tiles);
    *b = tiles < 2 ? 0 : levels_c2(k + 1, extent, tiles);
}
OCVAR_HD int levels_weight(int x, int a, int b) {
    const int p = 2 * x + 1;
    if (b <= a || p <= a) return 0;
    return p >= b ? 256 : ((p - a) * 256) / (b - a);
}

// Segments of an axis: every cell cut into pieces of at most `seg` pixels.
OCVAR_HD int levels_segments(int extent, int tiles, int seg) {
    int n = 0;
    for (int k = 0; k < levels_cells(tiles); k++)
        n += (levels_cell_start(k + 1, extent, tiles) - levels_cell_start(k, extent, tiles) + seg - 1) / seg;
    return n;
}
// Segment b < levels_segments(..): its cell, first pixel and length.
OCVAR_HD void levels_segment(int b, int extent, int tiles, int seg, int* cell, int* start, int* len) {
    *cell = 0, *start = 0, *len = 0;
    for (int k = 0; k < levels_cells(tiles); k++) {
        const int s = levels_cell_start(k, extent, tiles), e = levels_cell_start(k + 1, extent, tiles);
        const int n = (e - s + seg - 1) / seg;
        if (b < n) {
            *cell = k, *start = s + b * seg;
            *len = e - *start < seg ? e - *start : seg;
            return;
        }
        b -= n;
    }
}

// The gain cap on (lo, hi): afterwards hi - lo >= minr >= 1.
OCVAR_HD void levels_cap(int* lo, int* hi, int max_gain_q8) {
    const int minr = (255 * 256 + max_gain_q8 - 1) / max_gain_q8;
    if (*hi - *lo < minr) {
        int l = (*lo + *hi - minr) >> 1;
        l = l < 0 ? 0 : l;
        l = l > 255 - minr ? 255 - minr : l;
        *lo = l, *hi = l + minr;
    }
}

OCVAR_HD int levels_lut_value(int v, int lo, int hi) {
    int num = (v - lo) * 510 + (hi - lo);
    num = num < 0 ? 0 : num;
    const int q = num / (2 * (hi - lo));
    return q > 255 ? 255 : q;
}

OCVAR_HD unsigned long long levels_clip_count(unsigned n, int ppm) { return ((unsigned long long)n * (unsigned long long)ppm) / 1000000ull; }

// (lo, hi) of a histogram before the cap, sequentially.
inline void levels_bounds(const unsigned* hist, int low_ppm, int high_ppm, int* lo, int* hi) {
    unsigned n = 0;
    for (int v = 0; v < 256; v++) n += hist[v];
    const unsigned long long k_lo = levels_clip_count(n, low_ppm), k_hi = levels_clip_count(n, high_ppm);
    unsigned long long acc = 0;
    *lo = 255, *hi = 0;
    for (int v = 0; v < 256; v++) {
        acc += hist[v];
        if (acc > k_lo) {
            *lo = v;
            break;
        }
    }
    acc = 0;
    for (int v = 255; v >= 0; v--) {
        acc += hist[v];
        if (acc > k_hi) {
            *hi = v;
            break;
        }
    }
}

inline void levels_lut(const unsigned* hist, const OcvarLevelsParams& p, uint8_t* lut) {
    int lo, hi;
    levels_bounds(hist, p.low_ppm, p.high_ppm, &lo, &hi);
    levels_cap(&lo, &hi, p.max_gain_q8);
    for (int v = 0; v < 256; v++) lut[v] = (uint8_t)levels_lut_value(v, lo, hi);
}

// The blend of four LUT values.
OCVAR_HD int levels_mix(int t00, int t01, int t10, int t11, int wx, int wy) {
    const int top = t00 * (256 - wx) + t01 * wx, bot = t10 * (256 - wx) + t11 * wx;
    return (top * (256 - wy) + bot * wy + 32768) >> 16;
}

// One call's arguments, all pointers in device memory: frame f's pixels start *_frame_stride bytes after frame f - 1's, rows
// *_row_stride apart; the source is w x h pixels in the call's format, the destination w x h bytes; the two do not overlap.  hist
// and luts are the workspace's two halves (frame f's tile t at index f LEVELS_MAX_TILES + t); the host reference keeps its own.
struct LevelsArgs {
    const uint8_t* src;
    uint8_t* dst;
    int w, h;
    long long src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride;
    OcvarLevelsParams p;
    unsigned* hist;
    uint8_t* luts;
};

// The host reference: frame f of the call in format fmt, sequentially.  luts_out (may be nullptr) gets the frame's tiles_y tiles_x
// LUTs of 256 bytes, hist_out (may be nullptr) their histograms.
inline void levels_frame(const LevelsArgs& a, int fmt, int f, uint8_t* luts_out, unsigned* hist_out) {
    const int bpp = format_bpp(fmt), tx = a.p.tiles_x, ty = a.p.tiles_y;
    const uint8_t* src = a.src + (long long)f * a.src_frame_stride;
    uint8_t* dst = a.dst + (long long)f * a.dst_frame_stride;
    static thread_local unsigned hist[LEVELS_MAX_TILES][256];
    static thread_local uint8_t lut[LEVELS_MAX_TILES][256];
    const auto grey = [&](int x, int y) {
        const uint8_t* p = src + (long long)y * a.src_row_stride + (long long)x * bpp;
        return bpp == 1 ? (int)p[0] : levels_grey(p[0], p[1], p[2], fmt);
    };
    for (int j = 0; j < ty; j++)
        for (int i = 0; i < tx; i++) {
            unsigned* hh = hist[j * tx + i];
            for (int v = 0; v < 256; v++) hh[v] = 0;
            for (int y = levels_edge(j, a.h, ty); y < levels_edge(j + 1, a.h, ty); y++)
                for (int x = levels_edge(i, a.w, tx); x < levels_edge(i + 1, a.w, tx); x++) hh[grey(x, y)]++;
            levels_lut(hh, a.p, lut[j * tx + i]);
        }
    for (int y = 0; y < a.h; y++) {
        int j0, j1, wy;
        levels_axis(y, a.h, ty, &j0, &j1, &wy);
        for (int x = 0; x < a.w; x++) {
            int i0, i1, wx;
            levels_axis(x, a.w, tx, &i0, &i1, &wx);
            const int g = grey(x, y);
            dst[(long long)y * a.dst_row_stride + x] =
                (uint8_t)levels_mix(lut[j0 * tx + i0][g], lut[j0 * tx + i1][g], lut[j1 * tx + i0][g], lut[j1 * tx + i1][g], wx, wy);
        }
    }
    for (int t = 0; t < tx * ty; t++)
        for (int v = 0; v < 256; v++) {
            if (luts_out) luts_out[t * 256 + v] = lut[t][v];
            if (hist_out) hist_out[t * 256 + v] = hist[t][v];
        }
}

}  // namespace ocvar

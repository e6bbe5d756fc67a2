// levels_emul.cpp -- host build of the levels core (opencv-ar_amd/csrc/levels_core.h) for the levels tests: the sequential reference
// levels_emul, which the kernels of levels.hip must match byte for byte, with the LUTs and histograms it used, the pieces of the
// definition one by one, and the plan the kernels share with it: the apply kernel's segments and the histogram kernel's slabs.
// With -DLEVELS_EMUL_MAIN: a program that runs the extremes of the sizes, grids and parameters on heap blocks of exactly the bytes
// the call may touch, for a sanitizer build (g++ -fsanitize=address,undefined) run on its own.
#include "levels_core.h"

using namespace ocvar;

extern "C" {

// The call on n_frames frames; params NULL: the defaults.  luts (may be NULL) gets [n_frames][tiles][256] bytes, hist (may be NULL)
// as many counts.  Returns 0, or -2 (OCVAR_E_ARG) for what ocvar_hip_levels refuses of format, sizes, strides, n_frames and
// parameters, with nothing written.
int levels_emul(const uint8_t* src, int w, int h, long long src_row_stride, long long src_frame_stride, int format, uint8_t* dst,
                long long dst_row_stride, long long dst_frame_stride, int n_frames, const OcvarLevelsParams* params, uint8_t* luts, unsigned* hist) {
    OcvarLevelsParams p;
    levels_default_params(&p);
    if (params) p = *params;
    const int bpp = patch_bpp(format);
    if (bpp == 0 || w < 1 || w > LEVELS_MAX_SIDE || h < 1 || h > LEVELS_MAX_SIDE || n_frames < 1 || src_row_stride < (long long)bpp * w ||
        dst_row_stride < w || levels_params_bad(p, w, h))
        return OCVAR_E_ARG;
    const LevelsArgs a{src, dst, w, h, src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride, p, nullptr, nullptr};
    const size_t per = (size_t)p.tiles_x * p.tiles_y * 256;
    for (int f = 0; f < n_frames; f++) levels_frame(a, format, f, luts ? luts + f * per : nullptr, hist ? hist + f * per : nullptr);
    return OCVAR_OK;
}

void levels_default_params_emul(OcvarLevelsParams* p) { levels_default_params(p); }
int levels_params_bad_emul(const OcvarLevelsParams* p, int w, int h) { return levels_params_bad(*p, w, h); }

// The LUT of one histogram of 256 counts.
void levels_lut_emul(const unsigned* hist, const OcvarLevelsParams* p, uint8_t* lut) { levels_lut(hist, *p, lut); }

// out[0 .. 3]: lo and hi before the cap, lo and hi after it
void levels_bounds_emul(const unsigned* hist, const OcvarLevelsParams* p, int* out) {
    levels_bounds(hist, p->low_ppm, p->high_ppm, &out[0], &out[1]);
    out[2] = out[0], out[3] = out[1];
    levels_cap(&out[2], &out[3], p->max_gain_q8);
}

// out[0 .. 2]: i0, i1 and the weight of pixel x along an axis of `extent` pixels and `tiles` tiles
void levels_axis_emul(int x, int extent, int tiles, int* out) { levels_axis(x, extent, tiles, &out[0], &out[1], &out[2]); }

int levels_grey_emul(int c0, int c1, int c2, int fmt) { return levels_grey(c0, c1, c2, fmt); }

// The apply kernel's plan along one axis: the number of segments of at most seg pixels; out (may be NULL) gets cell, start, length
// of each.  Returns -1 when the segments do not cover 0 .. extent - 1 once and in order, each inside one cell, or when a pixel's
// cell or the weight the kernel computes for it differs from levels_axis.
int levels_segments_emul(int extent, int tiles, int seg, int* out) {
    const int n = levels_segments(extent, tiles, seg);
    int next = 0;
    for (int b = 0; b < n; b++) {
        int cell, start, len;
        levels_segment(b, extent, tiles, seg, &cell, &start, &len);
        if (start != next || len < 1 || len > seg) return -1;
        int a2, b2;
        levels_cell_centres(cell, extent, tiles, &a2, &b2);
        for (int x = start; x < start + len; x++) {
            int i0, i1, w;
            levels_axis(x, extent, tiles, &i0, &i1, &w);
            if (i0 != cell || i1 != (cell + 1 < tiles ? cell + 1 : tiles - 1) || w != levels_weight(x, a2, b2)) return -1;
        }
        next = start + len;
        if (out) out[3 * b] = cell, out[3 * b + 1] = start, out[3 * b + 2] = len;
    }
    return next == extent ? n : -1;
}

int levels_slab_rows_emul() { return LEVELS_SLAB_ROWS; }
int levels_seg_w_emul() { return LEVELS_SEG_W; }
int levels_seg_h_emul() { return LEVELS_SEG_H; }
int levels_ws_frames_emul() { return LEVELS_WS_FRAMES; }
long long levels_ws_bytes_emul() { return LEVELS_WS_BYTES; }

}  // extern "C"

#if defined(LEVELS_EMUL_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// One heap block per side, of exactly the bytes from its first to its last pixel byte: a byte read or written outside is the
// sanitizer's to report.  Rows carry a padding and frames a gap, whose bytes must keep their fill.
struct Block {
    uint8_t* p;
    long long row_bytes, rows, pitch, frame_stride, size;
    Block(long long row_bytes_, long long rows_, long long pad, long long gap, int n) : row_bytes(row_bytes_), rows(rows_) {
        pitch = row_bytes + pad;
        frame_stride = pitch * rows + gap;
        size = (n - 1) * frame_stride + (rows - 1) * pitch + row_bytes;
        p = (uint8_t*)malloc((size_t)size);
        memset(p, 0xA5, (size_t)size);
    }
    ~Block() { free(p); }
    bool padding_kept() const {
        for (long long o = 0; o < size; o++) {
            const long long in_frame = o % frame_stride;
            if ((in_frame >= pitch * rows || in_frame % pitch >= row_bytes) && p[o] != 0xA5) return false;
        }
        return true;
    }
};

// frame 0 random, frame 1 constant, frame 2 two-valued
static void fill(Block& b, int n, unsigned* seed) {
    for (int f = 0; f < n; f++)
        for (long long r = 0; r < b.rows; r++)
            for (long long k = 0; k < b.row_bytes; k++) {
                *seed = *seed * 1664525u + 1013904223u;
                b.p[f * b.frame_stride + r * b.pitch + k] = f == 0 ? (uint8_t)(*seed >> 24) : (f == 1 ? 255 : ((*seed >> 20) & 1 ? 250 : 3));
            }
}

static int sweep_case(int format, int w, int h, const OcvarLevelsParams& p) {
    const int bpp = patch_bpp(format), n = 3;
    unsigned seed = (unsigned)(format * 131 + w * 3 + h * 5 + p.tiles_x * 7 + p.tiles_y * 11 + p.low_ppm + p.max_gain_q8);
    Block src((long long)bpp * w, h, 3, 5, n), dst(w, h, 1, 7, n);
    fill(src, n, &seed);
    int bad = levels_emul(src.p, w, h, src.pitch, src.frame_stride, format, dst.p, dst.pitch, dst.frame_stride, n, &p, nullptr, nullptr) != OCVAR_OK;
    if (!dst.padding_kept()) bad++;
    // the constant frame: every tile's lo = hi = 255, capped, and 255 maps to 255
    for (long long r = 0; r < h; r++)
        for (long long x = 0; x < w; x++) bad += dst.p[dst.frame_stride + r * dst.pitch + x] != 255;
    bad += levels_segments_emul(w, p.tiles_x, LEVELS_SEG_W, nullptr) < 1 || levels_segments_emul(h, p.tiles_y, LEVELS_SEG_H, nullptr) < 1;
    return bad;
}

int main() {
    static const int sizes[][4] = {{1, 1, 1, 1},   {2, 1, 2, 1},   {5, 3, 1, 1},    {7, 3, 7, 1},     {16, 16, 8, 8},  {37, 23, 4, 3},
                                   {37, 23, 5, 2}, {67, 41, 8, 8}, {300, 64, 16, 4}, {32767, 1, 16, 1}, {1, 32767, 1, 16}, {32767, 2, 3, 2}};
    static const int knobs[][3] = {{10000, 10000, 2048}, {0, 0, 256}, {500000, 500000, 65280}, {0, 500000, 300}};
    int bad = 0, cases = 0;
    for (int format : {OCVAR_FMT_BGR, OCVAR_FMT_RGBA, OCVAR_FMT_GRAY})   // 3, 4 and 1 bytes per pixel
        for (const auto& s : sizes)
            for (const auto& k : knobs) {
                bad += sweep_case(format, s[0], s[1], OcvarLevelsParams{s[2], s[3], k[0], k[1], k[2]});
                cases++;
            }
    // refusals write nothing
    uint8_t px[12] = {0}, out[4] = {0xA5, 0xA5, 0xA5, 0xA5};
    const OcvarLevelsParams wrong[] = {{0, 1, 0, 0, 2048}, {17, 1, 0, 0, 2048}, {16, 5, 0, 0, 2048}, {3, 1, 0, 0, 2048}, {1, 3, 0, 0, 2048},
                                       {1, 1, -1, 0, 2048}, {1, 1, 0, 500001, 2048}, {1, 1, 0, 0, 255}, {1, 1, 0, 0, 65281}};
    for (const auto& p : wrong) bad += levels_emul(px, 2, 2, 6, 12, OCVAR_FMT_BGR, out, 2, 4, 1, &p, nullptr, nullptr) != OCVAR_E_ARG;
    bad += levels_emul(px, 2, 2, 6, 12, 5, out, 2, 4, 1, nullptr, nullptr, nullptr) != OCVAR_E_ARG;
    bad += levels_emul(px, 2, 2, 5, 12, OCVAR_FMT_BGR, out, 2, 4, 1, nullptr, nullptr, nullptr) != OCVAR_E_ARG;
    bad += levels_emul(px, 2, 2, 6, 12, OCVAR_FMT_BGR, out, 1, 4, 1, nullptr, nullptr, nullptr) != OCVAR_E_ARG;
    bad += levels_emul(px, 2, 2, 6, 12, OCVAR_FMT_BGR, out, 2, 4, 0, nullptr, nullptr, nullptr) != OCVAR_E_ARG;
    for (int i = 0; i < 4; i++) bad += out[i] != 0xA5;
    printf("levels_emul: %d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif

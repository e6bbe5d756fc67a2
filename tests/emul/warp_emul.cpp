// warp_emul.cpp -- host build of the warp core (opencv-ar_amd/csrc/warp_core.h) for the warp tests: the sequential references
// warp_emul, warp_records_emul and warp_board_plane_maps_emul, which the kernels of warp.hip must match byte for byte, the tile plan
// tile by tile with a count of its classes and of the taps its windows miss, and the patch reference (patch_core.h) with the map
// it used, for the equivalence test.  With -DWARP_EMUL_MAIN: a program that runs the extremes of the sizes and maps on heap blocks
// of exactly the bytes the calls may touch, for a sanitizer build (g++ -fsanitize=address,undefined) run on its own.
#include "warp_core.h"

using namespace ocvar;

extern "C" {

// The kernel's arguments, field by field, and the number of frames.  Returns the number of frames warped (status 1), or -2
// (OCVAR_E_ARG) for what ocvar_hip_warp refuses of format, sizes, interpolation, border and flags, with nothing written.
int warp_emul(const uint8_t* src, int sw, int sh, long long src_row_stride, long long src_frame_stride, uint8_t* dst, int dw, int dh,
              long long dst_row_stride, long long dst_frame_stride, int n_frames, int format, const double* maps, int interp, int border,
              const uint8_t* fill, int flags, int* status) {
    const auto side_ok = [](int v) { return v >= 1 && v <= WARP_MAX_SIDE; };
    if (patch_bpp(format) == 0 || !warp_interp_ok(interp) || !warp_border_ok(border) || (flags & ~WARP_FLAGS) || !side_ok(sw) || !side_ok(sh) ||
        !side_ok(dw) || !side_ok(dh) || n_frames < 1)
        return OCVAR_E_ARG;
    WarpArgs a{src, dst, sw, sh, dw, dh, src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride, maps, status, interp, border, flags, 0,
               {0, 0, 0, 0}};
    for (int k = 0; k < 4; k++) a.fill[k] = fill ? fill[k] : 0;
    return warp_frames(a, format, n_frames);
}

// 1 and M (destination -> source), or 0: the status rule on one map
int warp_map_emul(const double* m, int flags, double* M) { return warp_map(m, flags, M) ? 1 : 0; }

// out[0 .. 1]: the source position of destination pixel (x, y) in the interpolation's fixed point
void warp_source_emul(const double* M, int x, int y, int interp, int* out) { warp_source_fixed(M, x, y, warp_scale(interp), &out[0], &out[1]); }

// The record call on n_frames frames of `slots` records; cam may be NULL without OCVAR_WARP_POSE.  Returns 0, or -2 for what
// ocvar_hip_warp_records refuses of flags, with nothing written.
int warp_records_emul(const MarkerRec* in, const int* counts, int n_frames, int slots, const double* maps, int flags, const CameraRec* cam,
                      MarkerRec* out) {
    if ((flags & ~WARP_REC_FLAGS) || (flags & OCVAR_WARP_INVERSE_MAP) || ((flags & OCVAR_WARP_POSE) && !cam)) return OCVAR_E_ARG;
    const CameraRec none{};
    for (int f = 0; f < n_frames; f++)
        warp_records(in + (size_t)f * slots, counts[f], slots, (flags & OCVAR_WARP_ONE_MAP) ? maps : maps + 9 * (size_t)f, flags, cam ? *cam : none,
                     out + (size_t)f * slots);
    return OCVAR_OK;
}

void warp_board_plane_maps_emul(const OcvarBoardPose* poses, int n_frames, const double* K, const double* rect, int dw, int dh, double* maps) {
    for (int f = 0; f < n_frames; f++) warp_board_plane_map(poses[f], K, rect, dw, dh, maps + 9 * (size_t)f);
}

// out[0 .. 7]: staged, x0, y0, w, h, b0, row_dwords, pitch of one tile's plan
void warp_tile_plan_emul(const double* M, int tx0, int ty0, int tw, int th, int sw, int sh, int bpp, int interp, int budget_dwords, int* out) {
    const WarpPlan p = warp_tile_plan(M, tx0, ty0, tw, th, sw, sh, bpp, interp, budget_dwords);
    const int v[8] = {p.staged, p.x0, p.y0, p.w, p.h, p.b0, p.row_dwords, p.pitch};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}

// The kernel's tiles of one frame under map m: out[0] staged tiles, out[1] direct tiles, out[2] taps of pixels of staged tiles that
// lie inside the source (after the border rule) but outside the tile's window, out[3] taps looked at, out[4] the largest staged
// image in dwords.  Returns 0 for a skipped frame, else 1.
int warp_plan_count_emul(const double* m, int flags, int sw, int sh, int dw, int dh, int bpp, int interp, int border, long long* out) {
    double M[9];
    for (int i = 0; i < 5; i++) out[i] = 0;
    if (!warp_map(m, flags, M)) return 0;
    const int tile_h = warp_tile_h(bpp);
    for (int ty0 = 0; ty0 < dh; ty0 += tile_h)
        for (int tx0 = 0; tx0 < dw; tx0 += WARP_TILE_W) {
            const int tw = dw - tx0 < WARP_TILE_W ? dw - tx0 : WARP_TILE_W, th = dh - ty0 < tile_h ? dh - ty0 : tile_h;
            const WarpPlan p = warp_tile_plan(M, tx0, ty0, tw, th, sw, sh, bpp, interp, WARP_LDS_DWORDS);
            out[p.staged ? 0 : 1]++;
            if (!p.staged) continue;
            const long long words = (long long)p.h * p.pitch + 2;
            out[4] = words > out[4] ? words : out[4];
            for (int y = ty0; y < ty0 + th; y++)
                for (int x = tx0; x < tx0 + tw; x++) {
                    int X, Y;
                    warp_source_fixed(M, x, y, warp_scale(interp), &X, &Y);
                    warp_sample(
                        [&](int ix, int iy) -> int {
                            out[3]++;
                            if (ix < p.x0 || ix >= p.x0 + p.w || iy < p.y0 || iy >= p.y0 + p.h) out[2]++;
                            return 0;
                        },
                        sw, sh, X, Y, interp, border, 0);
                }
        }
    return 1;
}

// The patch reference on one record of one frame (patch_extract_frame, flags 0): the pw x ph patch and status, and in map[0 .. 8] the
// forward map it used, perspective_from_quad(square, pw, ph) widened to double (zeros when there is none).
int warp_patch_reference_emul(const uint8_t* frame, int W, int H, long long row_stride, int fmt, const MarkerRec* rec, int pw, int ph, uint8_t* patch,
                              double* map) {
    int status = 0;
    patch_extract_frame(frame, W, H, row_stride, fmt, rec, 1, 1, patch, pw, ph, 0, &status);
    float m32[9];
    const bool ok = perspective_from_quad(rec->square, pw, ph, m32);
    for (int i = 0; i < 9; i++) map[i] = ok ? (double)m32[i] : 0.0;
    return status;
}

// out[0 .. 1]: the core's own sine and cosine of theta >= 0
void warp_sincos_emul(double theta, double* out) { warp_sincos(theta, &out[0], &out[1]); }

int warp_tile_w_emul() { return WARP_TILE_W; }
int warp_tile_h_emul(int bpp) { return warp_tile_h(bpp); }
int warp_lds_dwords_emul() { return WARP_LDS_DWORDS; }

}  // extern "C"

#if defined(WARP_EMUL_MAIN)
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
    void fill(unsigned* seed, int n) {
        for (int f = 0; f < n; f++)
            for (long long r = 0; r < rows; r++)
                for (long long b = 0; b < row_bytes; b++) {
                    *seed = *seed * 1664525u + 1013904223u;
                    p[f * frame_stride + r * pitch + b] = (uint8_t)(*seed >> 24);
                }
    }
    bool padding_kept() const {
        for (long long o = 0; o < size; o++) {
            const long long in_frame = o % frame_stride;
            if ((in_frame >= pitch * rows || in_frame % pitch >= row_bytes) && p[o] != 0xA5) return false;
        }
        return true;
    }
};

// maps for a sw x sh source and a dw x dh destination: identity, a fit of the source into the destination, a magnification about
// the centre, a horizon through the destination, everything outside, a singular one and one with a NaN
static void make_maps(int sw, int sh, int dw, int dh, double (*m)[9]) {
    const double maps[7][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1},
                               {(double)dw / sw, 0, 0, 0, (double)dh / sh, 0, 0, 0, 1},
                               {3.5, 0.2, -1.25 * sw, -0.1, 3.25, -1.125 * sh, 0, 0, 1},
                               {1, 0.1, 0, 0.05, 1, 0, 2.0 / (dw + 1), 0, -1},
                               {1, 0, 1e7, 0, 1, -1e7, 0, 0, 1},
                               {1, 2, 3, 2, 4, 6, 0, 0, 1},
                               {1, 0, 0, 0, NAN, 0, 0, 0, 1}};
    memcpy(m, maps, sizeof(maps));
}

static int sweep_case(int format, int sw, int sh, int dw, int dh, int interp, int border) {
    const int bpp = patch_bpp(format), n = 7;
    unsigned seed = (unsigned)(format * 131 + sw * 3 + sh * 5 + dw * 7 + dh * 11 + interp + 2 * border);
    Block src((long long)bpp * sw, sh, 3, 5, n), dst((long long)bpp * dw, dh, 1, 7, n);
    src.fill(&seed, n);
    double maps[7][9];
    make_maps(sw, sh, dw, dh, maps);
    int status[7];
    const uint8_t fill[4] = {9, 99, 199, 29};
    int bad = warp_emul(src.p, sw, sh, src.pitch, src.frame_stride, dst.p, dw, dh, dst.pitch, dst.frame_stride, n, format, &maps[0][0], interp, border, fill,
                        0, status) != 5;
    if (!dst.padding_kept()) bad++;
    for (int f = 0; f < n; f++) bad += status[f] != (f < 5);
    // the skipped frames keep their bytes; the identity copies what both sides have and fills or replicates the rest
    for (int f = 5; f < n; f++)
        for (long long r = 0; r < dh; r++)
            for (long long b = 0; b < dst.row_bytes; b++) bad += dst.p[f * dst.frame_stride + r * dst.pitch + b] != 0xA5;
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++)
            for (int c = 0; c < bpp; c++) {
                const int xs = x < sw ? x : sw - 1, ys = y < sh ? y : sh - 1;
                const bool in = x < sw && y < sh;
                const int want = (in || border == OCVAR_WARP_BORDER_REPLICATE) ? src.p[ys * src.pitch + (long long)xs * bpp + c] : fill[c];
                bad += dst.p[y * dst.pitch + (long long)x * bpp + c] != want;
            }
    // the plan of every map: every tile has a class, and no staged window misses a tap
    for (int f = 0; f < 5; f++) {
        long long out[5];
        bad += warp_plan_count_emul(maps[f], 0, sw, sh, dw, dh, bpp, interp, border, out) != 1;
        bad += out[2] != 0 || out[4] > WARP_LDS_DWORDS;
    }
    return bad;
}

int main() {
    static const int sizes[][4] = {{1, 1, 1, 1},    {2, 1, 1, 1},     {1, 1, 2, 1},    {3, 2, 65, 17},  {7, 9, 63, 15},  {300, 200, 8, 8},
                                   {64, 16, 64, 16}, {129, 33, 65, 17}, {32767, 1, 5, 3}, {1, 32767, 3, 5}, {5, 3, 32767, 1}, {3, 5, 1, 32767}};
    int bad = 0, cases = 0;
    for (int format : {OCVAR_FMT_BGR, OCVAR_FMT_RGBA, OCVAR_FMT_GRAY})   // 3, 4 and 1 bytes per pixel
        for (const auto& s : sizes)
            for (int interp = 0; interp < 2; interp++)
                for (int border = 0; border < 2; border++) {
                    bad += sweep_case(format, s[0], s[1], s[2], s[3], interp, border);
                    cases++;
                }
    // records: every slot below the count, none above it; a corner on the horizon is the one NaN; a refusal writes nothing
    MarkerRec recs[4], out[4];
    memset(recs, 0, sizeof(recs));
    memset(out, 0xA5, sizeof(out));
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < 8; i++) recs[k].square[i] = (float)(k * 31 + i * 7) + 0.25f;
    const int counts[2] = {1, 5};
    const double m[9] = {2, 0, 1, 0, 2, 3, 1, 0, -0.25};   // w = x - 0.25: corner 0 of record 0 lies on the horizon
    bad += warp_records_emul(recs, counts, 2, 2, m, OCVAR_WARP_ONE_MAP, nullptr, out) != OCVAR_OK;
    const unsigned char* o1 = (const unsigned char*)&out[1];
    for (size_t i = 0; i < sizeof(MarkerRec); i++) bad += o1[i] != 0xA5;
    unsigned bits;
    memcpy(&bits, &out[0].square[0], 4);
    bad += bits != 0x7FC00000u;
    bad += out[0].square[2] != (float)((2 * 14.25 + 1) / 14.0) || out[3].square[7] != (float)((2 * 142.25 + 3) / (135.25 - 0.25));
    memset(out, 0xA5, sizeof(out));
    bad += warp_records_emul(recs, counts, 2, 2, m, OCVAR_WARP_ONE_MAP | OCVAR_WARP_INVERSE_MAP, nullptr, out) != OCVAR_E_ARG;
    bad += warp_records_emul(recs, counts, 2, 2, m, OCVAR_WARP_ONE_MAP | OCVAR_WARP_POSE, nullptr, out) != OCVAR_E_ARG;
    for (size_t i = 0; i < sizeof(out); i++) bad += ((const unsigned char*)out)[i] != 0xA5;
    // the plane map of a pose that is not solved: nine NaNs, and the warp skips it
    OcvarBoardPose pose{};
    pose.tvec[2] = 5;
    const double K[9] = {800, 0, 320, 0, 800, 240, 0, 0, 1}, rect[4] = {0, 0, 4, 3};
    double M[9];
    warp_board_plane_maps_emul(&pose, 1, K, rect, 64, 48, M);
    for (int i = 0; i < 9; i++) bad += M[i] == M[i];
    pose.status = 1;
    warp_board_plane_maps_emul(&pose, 1, K, rect, 64, 48, M);
    bad += M[2] != 320 * 5.0 || M[5] != 240 * 5.0 || M[8] != 5.0 || M[0] != 800 * (4.0 / 63);
    printf("warp_emul: %d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif

// yuv_emul.cpp -- host build of the YUV conversion core (opencv-ar_amd/csrc/yuv_core.h) for the yuv tests: the sequential
// references yuv_to_frames_emul and frames_to_yuv_emul, which the kernels of yuv.hip must match byte for byte, and the three
// formulas on all 2^24 inputs.  With -DYUV_EMUL_MAIN: a program that runs the layout sweep on heap blocks of exactly the bytes
// the conversions may touch, for a sanitizer build (g++ -fsanitize=address,undefined) run on its own.
#include "yuv_core.h"

using namespace ocvar;

static YuvArgs args_of(int layout, int matrix, const uint8_t* y, const uint8_t* c0, const uint8_t* c1, long long y_pitch, long long c_pitch,
                       long long yuv_frame_stride, const uint8_t* pix, long long pix_row_stride, long long pix_frame_stride, int W, int H,
                       int format) {
    return YuvArgs{const_cast<uint8_t*>(y), const_cast<uint8_t*>(c0), const_cast<uint8_t*>(c1), y_pitch, c_pitch, yuv_frame_stride,
                   const_cast<uint8_t*>(pix), pix_row_stride, pix_frame_stride, W, H, layout, format, yuv_coef(matrix)};
}

extern "C" {

// The kernels' arguments, field by field, and the number of frames: n_frames YUV frames to n_frames frames in `format`.
void yuv_to_frames_emul(int layout, int matrix, const uint8_t* y, const uint8_t* c0, const uint8_t* c1, long long y_pitch, long long c_pitch,
                        long long yuv_frame_stride, uint8_t* pix, long long pix_row_stride, long long pix_frame_stride, int W, int H, int format,
                        int n_frames) {
    const YuvArgs a = args_of(layout, matrix, y, c0, c1, y_pitch, c_pitch, yuv_frame_stride, pix, pix_row_stride, pix_frame_stride, W, H, format);
    for (int f = 0; f < n_frames; f++) yuv_to_frame(a, f);
}

// The other direction.
void frames_to_yuv_emul(int layout, int matrix, uint8_t* y, uint8_t* c0, uint8_t* c1, long long y_pitch, long long c_pitch,
                        long long yuv_frame_stride, const uint8_t* pix, long long pix_row_stride, long long pix_frame_stride, int W, int H,
                        int format, int n_frames) {
    const YuvArgs a = args_of(layout, matrix, y, c0, c1, y_pitch, c_pitch, yuv_frame_stride, pix, pix_row_stride, pix_frame_stride, W, H, format);
    for (int f = 0; f < n_frames; f++) frame_to_yuv(a, f);
}

// B G R of all 2^24 triples: out[((Y << 16) | (U << 8) | V) * 3 + 0 .. 2]
void yuv_to_bgr_all_emul(int matrix, uint8_t* out) {
    const YuvCoef k = yuv_coef(matrix);
    for (int i = 0; i < (1 << 24); i++) {
        int B, G, R;
        yuv_to_bgr(k, i >> 16, (i >> 8) & 255, i & 255, &B, &G, &R);
        out[3 * (size_t)i] = (uint8_t)B;
        out[3 * (size_t)i + 1] = (uint8_t)G;
        out[3 * (size_t)i + 2] = (uint8_t)R;
    }
}

// Y U V of all 2^24 colours as constant blocks of 2^log2n pixels: out[((B << 16) | (G << 8) | R) * 3 + 0 .. 2]; the values before
// the cast to a byte must fit one (returns the number that do not: 0)
int bgr_to_yuv_all_emul(int matrix, int log2n, uint8_t* out) {
    const YuvCoef k = yuv_coef(matrix);
    int bad = 0;
    for (int i = 0; i < (1 << 24); i++) {
        const int B = i >> 16, G = (i >> 8) & 255, R = i & 255;
        int U, V;
        const int Y = yuv_luma(k, B, G, R);
        yuv_chroma(k, B << log2n, G << log2n, R << log2n, log2n, &U, &V);
        bad += (Y | U | V) >> 8 ? 1 : 0;
        out[3 * (size_t)i] = (uint8_t)Y;
        out[3 * (size_t)i + 1] = (uint8_t)U;
        out[3 * (size_t)i + 2] = (uint8_t)V;
    }
    return bad;
}

// U V of n blocks from their channel sums: sums [n][3] ints (sB sG sR) -> out [n][2] bytes
void yuv_chroma_emul(int matrix, int log2n, const int* sums, int n, uint8_t* out) {
    const YuvCoef k = yuv_coef(matrix);
    for (int i = 0; i < n; i++) {
        int U, V;
        yuv_chroma(k, sums[3 * i], sums[3 * i + 1], sums[3 * i + 2], log2n, &U, &V);
        out[2 * i] = (uint8_t)U;
        out[2 * i + 1] = (uint8_t)V;
    }
}

// the 14 coefficients of a table, in YuvCoef's order
void yuv_coef_emul(int matrix, int* out) {
    const YuvCoef k = yuv_coef(matrix);
    const int v[14] = {k.cy, k.cub, k.cug, k.cvg, k.cvr, k.ry, k.gy, k.by, k.ru, k.gu, k.bu, k.rv, k.gv, k.bv};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}

}  // extern "C"

#if defined(YUV_EMUL_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// One heap block per plane and per frame block, each of exactly the bytes from its first to its last sample: a byte read or written
// outside is the sanitizer's to report.  Rows carry a padding and frames a gap, whose bytes must keep their fill.
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
    // the bytes between the rows and between the frames still hold the fill
    bool padding_kept() const {
        for (long long o = 0; o < size; o++) {
            const long long in_frame = o % frame_stride;
            if ((in_frame >= pitch * rows || in_frame % pitch >= row_bytes) && p[o] != 0xA5) return false;
        }
        return true;
    }
};

static int sweep_case(int layout, int matrix, int format, int W, int H, int n) {
    const int bpp = patch_bpp(format);
    const bool s420 = yuv_is_420(layout);
    unsigned seed = (unsigned)(layout * 131 + format * 17 + W * 3 + H);
    Block y(s420 ? W : 2 * W, H, 3, 5, n);
    // the chroma planes (one row of their own where the layout has none) lie in blocks of their own; a block's frames are as far
    // apart as the Y plane's, which is the one frame stride of the arguments
    const long long c_rows = s420 ? H / 2 : 1, c0_bytes = layout == OCVAR_YUV_NV12 ? W : W / 2, c1_bytes = W / 2;
    Block c0b(c0_bytes, c_rows, 1, y.frame_stride - (c0_bytes + 1) * c_rows, n), c1b(c1_bytes, c_rows, 1, y.frame_stride - (c1_bytes + 1) * c_rows, n);
    if (c0b.frame_stride != y.frame_stride || c1b.frame_stride != y.frame_stride) return 1;
    Block pix((long long)bpp * W, H, 1, 7, n), back((long long)bpp * W, H, 1, 7, n);
    y.fill(&seed, n);
    c0b.fill(&seed, n);
    c1b.fill(&seed, n);
    // YUV to colour, colour to YUV into fresh planes, and to colour again
    yuv_to_frames_emul(layout, matrix, y.p, c0b.p, c1b.p, y.pitch, c0b.pitch, y.frame_stride, pix.p, pix.pitch, pix.frame_stride, W, H, format, n);
    Block y2(y.row_bytes, H, 3, 5, n), u2(c0_bytes, c_rows, 1, y.frame_stride - (c0_bytes + 1) * c_rows, n),
        v2(c1_bytes, c_rows, 1, y.frame_stride - (c1_bytes + 1) * c_rows, n);
    frames_to_yuv_emul(layout, matrix, y2.p, u2.p, v2.p, y2.pitch, u2.pitch, y2.frame_stride, pix.p, pix.pitch, pix.frame_stride, W, H, format, n);
    yuv_to_frames_emul(layout, matrix, y2.p, u2.p, v2.p, y2.pitch, u2.pitch, y2.frame_stride, back.p, back.pitch, back.frame_stride, W, H, format, n);
    int bad = 0;
    if (!pix.padding_kept() || !back.padding_kept() || !y2.padding_kept()) bad++;
    if (s420 && (!u2.padding_kept() || (layout == OCVAR_YUV_I420 && !v2.padding_kept()))) bad++;
    if (bpp == 4)
        for (int f = 0; f < n; f++)
            for (int r = 0; r < H; r++)
                for (int x = 0; x < W; x++) bad += pix.p[f * pix.frame_stride + r * pix.pitch + 4 * x + 3] != 255;
    return bad;
}

int main() {
    static const int sizes[][2] = {{2, 2}, {4, 2}, {6, 4}, {8, 2}, {10, 6}, {510, 2}, {512, 4}, {514, 2}, {1026, 2}};
    int bad = 0, cases = 0;
    for (int layout = OCVAR_YUV_NV12; layout <= OCVAR_YUV_UYVY; layout++)
        for (int format = OCVAR_FMT_BGR; format <= OCVAR_FMT_GRAY; format++)
            for (const auto& s : sizes)
                for (int matrix = OCVAR_YUV_BT601; matrix <= OCVAR_YUV_BT709; matrix++) {
                    bad += sweep_case(layout, matrix, format, s[0], s[1], 2);
                    cases++;
                }
    printf("yuv_emul: %d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif

// yuv_ex_emul.cpp -- host build of the extended YUV conversion core (opencv-ar_amd/csrc/yuv_ex_core.h) for the yuv_ex tests: the
// two host calls yuv_ex_to_frames_emul and yuv_ex_from_frames_emul -- yuv_ex_check's refusals, then the sequential references,
// which the kernels of yuv_ex.hip must match byte for byte -- the tables, and the formulas on lists of inputs.  With
// -DYUV_EX_EMUL_MAIN: a program that runs the layout x depth x format sweep on heap blocks of exactly the bytes the conversions
// may touch, for a sanitizer build (g++ -fsanitize=address,undefined) run on its own.
#include "yuv_ex_core.h"

using namespace ocvar;

extern "C" {

// The entry point's arguments and the size limit: 0 and the frames converted, or the reason of the refusal (YuvExBad) and
// nothing written.
int yuv_ex_to_frames_emul(const OcvarYuvFramesEx* src, uint8_t* pix, int row_stride, size_t frame_stride, int W, int H, int n_frames, int format,
                          int max_w, int max_h) {
    if (int bad = yuv_ex_check(src, pix, row_stride, frame_stride, W, H, n_frames, format, max_w, max_h)) return bad;
    const YuvExArgs a = yuv_ex_args(*src, 0, pix, row_stride, frame_stride, W, H, format);
    for (int f = 0; f < n_frames; f++) yuv_ex_to_frame(a, f);
    return 0;
}

int yuv_ex_from_frames_emul(const uint8_t* pix, int row_stride, size_t frame_stride, const OcvarYuvFramesEx* dst, int W, int H, int n_frames,
                            int format, int max_w, int max_h) {
    if (int bad = yuv_ex_check(dst, pix, row_stride, frame_stride, W, H, n_frames, format, max_w, max_h)) return bad;
    const YuvExArgs a = yuv_ex_args(*dst, 0, pix, row_stride, frame_stride, W, H, format);
    for (int f = 0; f < n_frames; f++) yuv_ex_from_frame(a, f);
    return 0;
}

// a table: the 14 coefficients in YuvCoef's order, then y_off, c_mid, out_y_off, out_shift, word_shift
void yuv_ex_coef_emul(int matrix, int range, int bits, int* out) {
    const YuvCoefEx t = yuv_coef_ex(matrix, range, bits);
    const YuvCoef& k = t.k;
    const int v[19] = {k.cy, k.cub, k.cug, k.cvg, k.cvr, k.ry, k.gy, k.by, k.ru, k.gu, k.bu, k.rv, k.gv, k.bv,
                       t.y_off, t.c_mid, t.out_y_off, t.out_shift, t.word_shift};
    for (int i = 0; i < 19; i++) out[i] = v[i];
}

// B G R of n triples of samples: yuv [n][3] uint16 (Y U V) -> out [n][3] bytes
void yuv_ex_to_bgr_emul(int matrix, int range, int bits, const uint16_t* yuv, long long n, uint8_t* out) {
    const YuvCoefEx k = yuv_coef_ex(matrix, range, bits);
    for (long long i = 0; i < n; i++) {
        int B, G, R;
        yuv_ex_to_bgr(k, yuv[3 * i], yuv[3 * i + 1], yuv[3 * i + 2], &B, &G, &R);
        out[3 * i] = (uint8_t)B;
        out[3 * i + 1] = (uint8_t)G;
        out[3 * i + 2] = (uint8_t)R;
    }
}

// Y U V of n colours as constant blocks of 2^log2n pixels: bgr [n][3] bytes -> out [n][3] uint16; the values before the cast must
// lie in 0 .. 2^bits - 1 (returns the number that do not: 0)
long long yuv_ex_from_bgr_emul(int matrix, int range, int bits, int log2n, const uint8_t* bgr, long long n, uint16_t* out) {
    const YuvCoefEx k = yuv_coef_ex(matrix, range, bits);
    long long bad = 0;
    for (long long i = 0; i < n; i++) {
        const int B = bgr[3 * i], G = bgr[3 * i + 1], R = bgr[3 * i + 2];
        int U, V;
        const int Y = yuv_ex_luma(k, B, G, R);
        yuv_ex_chroma(k, B << log2n, G << log2n, R << log2n, log2n, &U, &V);
        bad += ((Y | U | V) >> bits) ? 1 : 0;
        out[3 * i] = (uint16_t)Y;
        out[3 * i + 1] = (uint16_t)U;
        out[3 * i + 2] = (uint16_t)V;
    }
    return bad;
}

// U V of n blocks from their channel sums: sums [n][3] ints (sB sG sR) -> out [n][2] uint16
void yuv_ex_chroma_emul(int matrix, int range, int bits, int log2n, const int* sums, long long n, uint16_t* out) {
    const YuvCoefEx k = yuv_coef_ex(matrix, range, bits);
    for (long long i = 0; i < n; i++) {
        int U, V;
        yuv_ex_chroma(k, sums[3 * i], sums[3 * i + 1], sums[3 * i + 2], log2n, &U, &V);
        out[2 * i] = (uint16_t)U;
        out[2 * i + 1] = (uint16_t)V;
    }
}

}  // extern "C"

#if defined(YUV_EX_EMUL_MAIN)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// One heap block per plane and per frame block, each of exactly the bytes from its first to its last sample: a byte read or written
// outside is the sanitizer's to report.  Rows carry a padding and frames a gap, whose bytes must keep their fill.
struct Block {
    uint8_t* p;
    long long row_bytes, rows, pitch, frame_stride, size;
    Block(long long row_bytes_, long long rows_, long long pad, long long frame_stride_, int n) : row_bytes(row_bytes_), rows(rows_) {
        pitch = row_bytes + pad;
        frame_stride = frame_stride_;
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

static int sweep_case(int layout, int bits, int matrix, int range, int format, int W, int H, int n) {
    const int bpp = format_bpp(format), sub = yuv_ex_sub(layout), sb = bits > 8 ? 2 : 1;
    unsigned seed = (unsigned)(layout * 131 + format * 17 + W * 3 + H + bits);
    // every plane in a block of its own; the blocks' frames are as far apart as the largest plane needs, which is the one frame
    // stride of the descriptor.  Paddings are even, so that 16-bit samples stay at even addresses.
    const long long y_bytes = sub == YUV_SUB_422 ? 2 * W : (long long)W * sb;
    const long long c_rows = sub == YUV_SUB_420 ? H / 2 : (sub == YUV_SUB_444 ? H : 1);
    const long long c_bytes = yuv_ex_semiplanar(layout) ? (long long)W * sb : (sub == YUV_SUB_444 ? W : (W / 2 > 0 ? W / 2 : 1));
    const long long stride = (y_bytes + 4) * H + 6;
    Block y(y_bytes, H, 4, stride, n), c0b(c_bytes, c_rows, 2, stride, n), c1b(c_bytes, c_rows, 2, stride, n);
    Block pix((long long)bpp * W, H, 1, ((long long)bpp * W + 1) * H + 7, n), back((long long)bpp * W, H, 1, ((long long)bpp * W + 1) * H + 7, n);
    y.fill(&seed, n);
    c0b.fill(&seed, n);
    c1b.fill(&seed, n);
    const OcvarYuvFramesEx src{layout, matrix, range, bits, y.p, c0b.p, c1b.p, (int)y.pitch, (int)c0b.pitch, (size_t)stride};
    // YUV to colour, colour to YUV into fresh planes, and to colour again
    int bad = 0;
    bad += yuv_ex_to_frames_emul(&src, pix.p, (int)pix.pitch, (size_t)pix.frame_stride, W, H, n, format, 32767, 32767) != 0;
    Block y2(y_bytes, H, 4, stride, n), u2(c_bytes, c_rows, 2, stride, n), v2(c_bytes, c_rows, 2, stride, n);
    const OcvarYuvFramesEx dst{layout, matrix, range, bits, y2.p, u2.p, v2.p, (int)y2.pitch, (int)u2.pitch, (size_t)stride};
    bad += yuv_ex_from_frames_emul(pix.p, (int)pix.pitch, (size_t)pix.frame_stride, &dst, W, H, n, format, 32767, 32767) != 0;
    bad += yuv_ex_to_frames_emul(&dst, back.p, (int)back.pitch, (size_t)back.frame_stride, W, H, n, format, 32767, 32767) != 0;
    if (!pix.padding_kept() || !back.padding_kept() || !y2.padding_kept()) bad++;
    if (sub != YUV_SUB_422 && !u2.padding_kept()) bad++;
    if (!yuv_ex_semiplanar(layout) && sub != YUV_SUB_422 && !v2.padding_kept()) bad++;
    if (bpp == 4)
        for (int f = 0; f < n; f++)
            for (int r = 0; r < H; r++)
                for (int x = 0; x < W; x++) bad += pix.p[f * pix.frame_stride + r * pix.pitch + 4 * x + 3] != 255;
    if (sb == 2)   // the low bits of every word written are zero
        for (int f = 0; f < n; f++)
            for (int r = 0; r < H; r++)
                for (int x = 0; x < W; x++) bad += (*(const uint16_t*)(y2.p + f * stride + r * y2.pitch + 2 * x) & ((1 << (16 - bits)) - 1)) != 0;
    return bad;
}

int main() {
    static const int sizes[][2] = {{2, 2}, {4, 2}, {6, 4}, {8, 2}, {10, 6}, {510, 2}, {512, 4}, {514, 2}, {1026, 2}};
    static const int sizes444[][2] = {{1, 1}, {3, 3}, {7, 5}, {513, 3}, {1027, 1}};
    int bad = 0, cases = 0, k = 0;
    for (int layout = OCVAR_YUV_NV12; layout <= OCVAR_YUV_I444; layout++)
        for (int bits : {8, 10, 12, 16}) {
            if (bits > 8 && layout != OCVAR_YUV_NV12) continue;
            for (int format = OCVAR_FMT_BGR; format <= OCVAR_FMT_GRAY; format++) {
                for (const auto& s : sizes) {
                    bad += sweep_case(layout, bits, k % 3, (k / 3) % 2, format, s[0], s[1], 2);
                    cases++, k++;
                }
                if (layout == OCVAR_YUV_I444)
                    for (const auto& s : sizes444) {
                        bad += sweep_case(layout, bits, k % 3, (k / 3) % 2, format, s[0], s[1], 2);
                        cases++, k++;
                    }
            }
        }
    printf("yuv_ex_emul: %d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif

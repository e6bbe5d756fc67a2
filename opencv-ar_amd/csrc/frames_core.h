// frames_core.h -- what every frame operation asks of a block of frames in the caller's memory before a kernel may touch it:
// the formats' bytes per pixel, the bytes a block covers, whether two blocks share a byte, and the one check of sides, count,
// row stride and row span.  Plain arithmetic for host and device alike (tests/emul/frames_emul.cpp builds it with g++;
// tests/test_frames_cpu.py holds it to the same rules in unbounded integers); frame_ops.hip turns the reasons into error texts.
// (The frame binarise kernel's own addressing rule is another question: hd.h::frame_src_addressable.)
#pragma once
#include "hd.h"

namespace ocvar {

// bytes per pixel of a frame format (OCVAR_FMT_BGR 0, RGB 1, BGRA 2, RGBA 3, GRAY 4: frame_ops.hip asserts the values), 0: unknown
OCVAR_HD constexpr int format_bpp(int fmt) { return (fmt == 0 || fmt == 1) ? 3 : ((fmt == 2 || fmt == 3) ? 4 : (fmt == 4 ? 1 : 0)); }
// (the earlier name, for the host builds under tests/emul alone, which predate this header; product sources use format_bpp)
OCVAR_HD constexpr int patch_bpp(int fmt) { return format_bpp(fmt); }

// n_frames frames of width x height pixels of bpp bytes, rows row_stride and frames frame_stride bytes apart, from byte p on
struct FrameBlock {
    const uint8_t* p;
    int width, height, bpp;
    long long row_stride;
    unsigned long long frame_stride;
    int n_frames;
};

constexpr long long FRAMES_MAX_SPAN = 2147483647LL;   // the kernels' row offsets are 32-bit

// the bytes from a frame's first to its last pixel byte; from the block's (the stride of a single frame does not count)
OCVAR_HD long long frames_row_span(const FrameBlock& b) { return (long long)(b.height - 1) * b.row_stride + (long long)b.bpp * b.width; }
OCVAR_HD unsigned long long frames_extent(const FrameBlock& b) {
    return (unsigned long long)(b.n_frames - 1) * b.frame_stride + (unsigned long long)frames_row_span(b);
}

// whether the byte ranges of two blocks share a byte (gaps between rows and frames count as the block's)
OCVAR_HD bool frames_intersect(const FrameBlock& a, const FrameBlock& b) {
    const unsigned long long a0 = (unsigned long long)(uintptr_t)a.p, b0 = (unsigned long long)(uintptr_t)b.p;
    return a0 < b0 + frames_extent(b) && b0 < a0 + frames_extent(a);
}

// Why a block is refused, in the order the faults are looked for.  bpp 0 is format_bpp's unknown format; the sides are 1 ..
// max_w and 1 .. max_h (the context's size for some operations, 32767 for others: the caller says).
enum FramesBad { FRAMES_OK = 0, FRAMES_FORMAT, FRAMES_SIDE, FRAMES_COUNT, FRAMES_ROW_STRIDE, FRAMES_SPAN };
OCVAR_HD int frames_check(const FrameBlock& b, int max_w, int max_h) {
    if (b.bpp < 1) return FRAMES_FORMAT;
    if (b.width < 1 || b.height < 1 || b.width > max_w || b.height > max_h) return FRAMES_SIDE;
    if (b.n_frames < 1) return FRAMES_COUNT;
    if (b.row_stride < (long long)b.bpp * b.width) return FRAMES_ROW_STRIDE;
    if (frames_row_span(b) > FRAMES_MAX_SPAN) return FRAMES_SPAN;
    return FRAMES_OK;
}

// whether a block's first byte, rows and frames all lie at multiples of 4: the launchers' choice of the dword kernels
OCVAR_HD bool frames_dwords(const void* p, long long row_stride, long long frame_stride) {
    return (((unsigned long long)(uintptr_t)p | (unsigned long long)row_stride | (unsigned long long)frame_stride) & 3ull) == 0;
}

}  // namespace ocvar

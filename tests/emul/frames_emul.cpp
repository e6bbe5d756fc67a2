// frames_emul.cpp -- host build of the frame-block rules (opencv-ar_amd/csrc/frames_core.h) for tests/test_frames_cpu.py.
// TEST ONLY: nothing in the product links this.  With -DFRAMES_EMUL_MAIN it is a program that walks the same boundaries, for a
// run under -fsanitize=address,undefined.
#include "frames_core.h"

using namespace ocvar;

// a block as the test passes it: the first byte as a number
struct BlockIn {
    unsigned long long p;
    int width, height, bpp;
    long long row_stride;
    unsigned long long frame_stride;
    int n_frames;
};
static FrameBlock block(const BlockIn& b) {
    return FrameBlock{reinterpret_cast<const uint8_t*>((uintptr_t)b.p), b.width, b.height, b.bpp, b.row_stride, b.frame_stride, b.n_frames};
}

extern "C" int frames_emul_bpp(int fmt) { return format_bpp(fmt); }
extern "C" long long frames_emul_row_span(const BlockIn* b) { return frames_row_span(block(*b)); }
extern "C" unsigned long long frames_emul_extent(const BlockIn* b) { return frames_extent(block(*b)); }
extern "C" int frames_emul_intersect(const BlockIn* a, const BlockIn* b) { return frames_intersect(block(*a), block(*b)) ? 1 : 0; }
extern "C" int frames_emul_check(const BlockIn* b, int max_w, int max_h) { return frames_check(block(*b), max_w, max_h); }
extern "C" int frames_emul_dwords(unsigned long long p, long long row_stride, long long frame_stride) {
    return frames_dwords(reinterpret_cast<const void*>((uintptr_t)p), row_stride, frame_stride) ? 1 : 0;
}

#ifdef FRAMES_EMUL_MAIN
#include <cstdio>
#include <initializer_list>

static int failures = 0;
static void expect(bool ok, const char* what, long long a, long long b, long long c) {
    if (ok) return;
    failures++;
    std::printf("FAILED %s (%lld, %lld, %lld)\n", what, a, b, c);
}

int main() {
    const unsigned long long base = 1ull << 40;
    for (int fmt = -2; fmt <= 7; fmt++) expect(format_bpp(fmt) == (fmt < 0 || fmt > 4 ? 0 : fmt < 2 ? 3 : fmt < 4 ? 4 : 1), "format_bpp", fmt, 0, 0);
    const int bpps[] = {1, 3, 4}, widths[] = {1, 32767}, heights[] = {1, 2, 32767}, limits[] = {640, 32767};
    for (int bpp : bpps) {
        for (int w : widths) {
            BlockIn b{base, w, 2, bpp, (long long)bpp * w - 1, 0, 1};
            expect(frames_emul_check(&b, 32767, 32767) == FRAMES_ROW_STRIDE, "row stride below", bpp, w, 0);
            b.row_stride++;
            expect(frames_emul_check(&b, 32767, 32767) == FRAMES_OK, "row stride at", bpp, w, 0);
        }
        for (int h : heights) {
            const int w = 640;
            // the largest row stride whose span is within the limit (any, for one row), and one more
            const long long at = h == 1 ? 2147483647LL : (FRAMES_MAX_SPAN - (long long)bpp * w) / (h - 1);
            BlockIn b{base, w, h, bpp, at, 0, 1};
            expect(frames_emul_check(&b, 32767, 32767) == FRAMES_OK, "span at the limit", bpp, h, at);
            if (h == 2) expect(frames_emul_row_span(&b) == FRAMES_MAX_SPAN, "span exactly", bpp, h, at);
            if (h > 1) {
                b.row_stride++;
                expect(frames_emul_check(&b, 32767, 32767) == FRAMES_SPAN, "span above the limit", bpp, h, at + 1);
            }
        }
    }
    for (int lim : limits) {
        const int sides[] = {0, 1, lim, lim + 1};
        for (int s : sides) {
            const int want = s >= 1 && s <= lim ? FRAMES_OK : FRAMES_SIDE;
            BlockIn b{base, s, 1, 1, 65536, 0, 1}, d{base, 1, s, 1, 1, 0, 1};
            expect(frames_emul_check(&b, lim, lim) == want, "width", lim, s, 0);
            expect(frames_emul_check(&d, lim, lim) == want, "height", lim, s, 0);
        }
    }
    for (int n : {0, -1}) {
        BlockIn b{base, 4, 4, 1, 4, 16, n};
        expect(frames_emul_check(&b, 32767, 32767) == FRAMES_COUNT, "n_frames", n, 0, 0);
    }
    for (unsigned long long fs : {0ull, 1ull << 40}) {
        BlockIn b{base, 5, 3, 3, 20, fs, 1};
        expect(frames_emul_extent(&b) == 2 * 20 + 15, "extent of one frame", (long long)fs, 0, 0);
    }
    BlockIn three{base, 5, 3, 3, 20, 1000, 3};
    expect(frames_emul_extent(&three) == 2 * 1000 + 2 * 20 + 15, "extent of three frames", 0, 0, 0);
    // source 640 x 480 BGR, destination GRAY (levels) or turned (orient): touching, and one byte less
    BlockIn src{base, 640, 480, 3, 1920, 1920 * 480, 2};
    const unsigned long long src_end = base + frames_emul_extent(&src);
    const BlockIn dsts[] = {{0, 640, 480, 1, 640, 640 * 480, 2}, {0, 480, 640, 3, 1440, 1440 * 640, 2}, {0, 640, 480, 3, 1920, 1920 * 480, 2}};
    for (BlockIn d : dsts) {
        d.p = src_end;
        expect(!frames_emul_intersect(&src, &d) && !frames_emul_intersect(&d, &src), "behind, touching", d.bpp, d.width, 0);
        d.p = src_end - 1;
        expect(frames_emul_intersect(&src, &d) && frames_emul_intersect(&d, &src), "behind, one byte shared", d.bpp, d.width, 0);
        d.p = base - frames_emul_extent(&d);
        expect(!frames_emul_intersect(&src, &d) && !frames_emul_intersect(&d, &src), "in front, touching", d.bpp, d.width, 0);
        d.p++;
        expect(frames_emul_intersect(&src, &d) && frames_emul_intersect(&d, &src), "in front, one byte shared", d.bpp, d.width, 0);
    }
    BlockIn inner{base + 1920 * 10 + 30, 16, 16, 3, 1920, 0, 1};
    expect(frames_emul_intersect(&src, &inner) && frames_emul_intersect(&inner, &src) && frames_emul_intersect(&src, &src), "inside, identical", 0, 0, 0);
    for (int odd = 1; odd <= 3; odd++) {
        expect(!frames_emul_dwords(base + odd, 64, 4096) && !frames_emul_dwords(base, 64 + odd, 4096) && !frames_emul_dwords(base, 64, 4096 + odd),
               "dwords", odd, 0, 0);
    }
    expect(frames_emul_dwords(base, 64, 4096) && frames_emul_dwords(base, 64, 0), "dwords aligned", 0, 0, 0);
    std::printf(failures ? "frames_emul: %d failures\n" : "frames_emul: all boundaries hold\n", failures);
    return failures ? 1 : 0;
}
#endif

// Thin exports of hd.h's address arithmetic (tile offsets of the bit plane, the row division, the frame kernel's addressing
// rule) and of trace_core.h::mul_small, for tests/test_geometry_limits_cpu.py: each is compared with plain integer arithmetic over
// the whole range of sizes the C ABI admits.  Built with -DOCVAR_NBR_TILED, the product's plane layout.  (The grey plane's
// gray_col / gray_pitch are exported by emul.cpp.)
#include "hd.h"
#include "trace_core.h"

using namespace ocvar;

extern "C" unsigned geo_div14(unsigned y) { return div14(y); }
extern "C" void geo_div14_range(unsigned y0, unsigned y1, unsigned* out) {
    for (unsigned y = y0; y < y1; y++) out[y - y0] = div14(y);
}
extern "C" long long geo_plane_bytes(int ns, int sh) { return nbr_plane_bytes(ns, sh); }
extern "C" unsigned geo_tile_off(unsigned tx, unsigned ty, int ns) { return nbr_tile_off(tx, ty, ns); }
// window offsets of n points by both routes: (x, y, ns) and the followers' packed point with nt = ns / 16
extern "C" void geo_win_offs(int n, const int* x, const int* y, int ns, unsigned* by_xy, unsigned* by_packed) {
    for (int i = 0; i < n; i++) {
        by_xy[i] = nbr_win_off(x[i], y[i], ns);
        by_packed[i] = nbr_win_off_xy((unsigned)x[i] | ((unsigned)y[i] << 16), (unsigned)ns >> 4);
    }
}
extern "C" int geo_mul_small(int d, int ns) { return mul_small(d, ns); }
extern "C" int geo_frame_src_addressable(int width, int height, long long row_stride, int bpp) {
    return frame_src_addressable(width, height, row_stride, bpp) ? 1 : 0;
}
extern "C" long long geo_march_src_bytes() { return MARCH_SRC_BYTES; }

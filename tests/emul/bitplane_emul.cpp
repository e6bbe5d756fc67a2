// bitplane_emul.cpp -- host build of the neighbour-plane readers for tests/test_bitplane_cpu.py.  TEST ONLY.
//
// Compiled twice: with -DOCVAR_NBR_TILED (the product's bit plane: 16x14 tiles with a one-pixel apron, hd.h) and without
// (the raster byte plane of the host emulation).  Both builds export the same functions; the test runs the followers of
// trace_core.h on the same binary images in both and compares what they return.
#include "trace_core.h"
#include "plane_writer.h"
#include <vector>

using namespace ocvar;

static int bin_at(const uint8_t* bin, int w, int h, int x, int y) { return emul_bin_at(bin, w, h, x, y); }

extern "C" int bp_ns(int sw) { return emul_plane_ns(sw); }

extern "C" long long bp_plane_bytes(int sw, int sh) { return nbr_plane_bytes(bp_ns(sw), sh); }

extern "C" void bp_make_plane(const uint8_t* bin, int sw, int sh, uint8_t* plane) { emul_make_plane(bin, sw, sh, plane); }

// mask byte of every pixel through the build's reader (nbr_at), and -- bit plane -- through the followers' packed-point
// address (nbr_win_off_xy) and the own-pixel bit; returns the number of pixels where a reader disagrees with the definition
extern "C" long long bp_check_readers(const uint8_t* bin, int sw, int sh, const uint8_t* plane, uint8_t* masks) {
    const int ns = bp_ns(sw);
    long long bad = 0;
    for (int y = 0; y < sh; y++)
        for (int x = 0; x < sw; x++) {
            unsigned m = 0;
            for (int s = 0; s < 8; s++) m |= (unsigned)bin_at(bin, sw, sh, x + dir_dx(s), y + dir_dy(s)) << s;
            const unsigned got = nbr_at(plane, x, y, ns);
            masks[(size_t)y * sw + x] = (uint8_t)got;
            bad += got != m;
#if defined(OCVAR_NBR_TILED)
            const unsigned* w = reinterpret_cast<const unsigned*>(plane + nbr_win_off_xy((unsigned)x | ((unsigned)y << 16), (unsigned)ns >> 4));
            bad += nbr_mask9(w[0], w[1], w[2], (unsigned)x & 15u) != m;
            bad += nbr_bit(plane, x, y, ns) != (unsigned)bin_at(bin, sw, sh, x, y);
#endif
        }
    return bad;
}

// Every plausible border start of the image (cvFindContours' outer / hole start conditions), through every reader of the
// followers in trace_core.h: the run test, the look behind, the flat walk (tier 1's probe), trace_border without run skipping
// (tier 2's overflow path), and the two forms no kernel runs, kept as the tests' references: the lean walk and trace_border
// with run skipping.  (Tier 2's own step and tier 3's window are walk_core.h's: follow_emul.cpp, test_follow_tiers_cpu.py.)
// Per start 16 ints: position, kind, then the results; the walks' points go into a running hash.
extern "C" int bp_walks(const uint8_t* bin, int sw, int sh, const uint8_t* plane, int* out, int max_starts) {
    const int ns = bp_ns(sw), plane_pos = ns * sh;
    std::vector<int> pts(2 * (4 * (size_t)sw * sh + 16));
    const int max_pts = (int)pts.size() / 2 - 1, steps = 4 * sw * sh + 16;
    auto hash = [&](int n) {
        unsigned h = 2166136261u;
        for (int i = 0; i < 2 * n && i < 2 * max_pts; i++) h = (h ^ (unsigned)pts[i]) * 16777619u;
        return (int)h;
    };
    int n = 0;
    for (int y = 1; y < sh - 1; y++)
        for (int x = 1; x < sw - 1; x++) {
            const int c = bin_at(bin, sw, sh, x, y), wv = bin_at(bin, sw, sh, x - 1, y);
            if (c == wv) continue;
            const int hole = c ? 0 : 1, cpos = y * ns + x;
            if (n >= max_starts) return -1;
            int* o = out + 16 * (size_t)n++;
            o[0] = cpos;
            o[1] = hole;
            o[2] = run_has_earlier_pixel(plane, ns, cpos, hole, 16);
#if defined(OCVAR_NBR_TILED)
            o[3] = run_has_earlier_pixel_bits(plane, ns, cpos, hole);
#else
            o[3] = o[2];
#endif
            o[4] = earlier_start_behind(plane, ns, plane_pos, cpos, hole, 32);
            const LeanTrace a = trace_flat(plane, ns, plane_pos, cpos, hole, pts.data(), max_pts, steps);
            o[5] = a.status; o[6] = a.npts; o[7] = a.steps; o[8] = hash(a.npts);
            const LeanTrace b = trace_lean(plane, ns, plane_pos, cpos, hole, pts.data(), max_pts, steps);
            o[9] = b.status; o[10] = b.npts; o[11] = hash(b.npts);
            const TraceStats t = trace_border<true, false>(plane, ns, plane_pos, cpos, hole, pts.data(), max_pts, steps);
            o[12] = t.status; o[13] = t.npts; o[14] = hash(t.npts);
            const TraceStats r = trace_border<true, true>(plane, ns, plane_pos, cpos, hole, pts.data(), max_pts, steps);
            o[15] = (r.status == t.status && r.npts == t.npts && hash(r.npts) == o[14]) ? 1 : 0;
        }
    return n;
}

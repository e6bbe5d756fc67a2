// walk_core.h -- the arithmetic of follower tiers 2 and 3 (follow.hip) on the bit plane, free of HIP calls: tier 2's whole
// step (one lane per border) and its budget, and of tier 3 (one wave per border) the window's geometry, its load mapping, the
// mask read and the step decode.
// follow.hip's kernels use these; tests/emul/follow_emul.cpp builds them for the host and walks every plausible start of its
// images with them (tests/test_follow_tiers_cpu.py, against trace_flat and trace_border).  What stays in follow.hip is what
// needs a wave: tier 2's LDS parking, flushing and hand-out, and the loop of trace_lean_tiled with its ballots.
//
// The helpers are cut where the kernels' device code stays what it was, instruction for instruction: pointer arithmetic keeps the
// kernels' own chain of additions (hence helpers that return pointers), and a test of more than two terms is left to the caller
// to combine from two-term helpers -- folded into one function the same test compiled to differently ordered code for
// follow_long_kernel.  Compare the assembly of follow.hip before and after changing a signature here.
#pragma once
#include "trace_core.h"
#include "croplist_core.h"

#if !defined(OCVAR_NBR_TILED)
#error "walk_core.h reads the bit plane: build with -DOCVAR_NBR_TILED"
#endif

namespace ocvar {

// ---- the follower's step from a table (tier 2) ------------------------------------------------------------------------------
// trace_core.h::flat_step_t spends ~70 vector instructions per step: the rotate / count-trailing-zeros / rotate-back that turn
// (arrival direction, neighbour mask) into (exit direction, neighbours passed on the way), two table extractions for the
// direction's dx and dy, the scan position y * ns + x carried next to x and y, the tiled address from scratch, and a chain of
// selects.  The step is rebuilt around three ideas:
//  * the mask only matters through t = the number of zero neighbours examined before the next border pixel (a byte replicate,
//    a funnel shift and a find-first-bit), and everything the step decides is a function of (first examined direction, t): 64
//    states, ONE lookup in a 256-byte LDS table: entry = (dx + 1) | (dy + 1) << 16 | next first direction << 5 | exit
//    direction << 10 | passed-E << 30 | passed-W << 31.  (A table over (direction, mask) itself -- 8 KB per workgroup -- saved
//    four more instructions and cost a workgroup of occupancy next to the binarise kernels: slower.)
//  * the position is the packed point x | y << 16 itself (what is parked and stored anyway): one add3 moves it, and because y
//    is the major half, packed points compare like scan positions y * ns + x -- the "a position of this border before its
//    start" tests and the closing test need no scan position at all (passed-W / passed-E sit in the sign bits: an AND with the
//    signed distance to the start position decides).
//  * a walk that ends is never stepped again, so nothing is guarded.
// ~42 vector instructions per step instead of ~70; same states, same points, same status as flat_step_t, step for step
// (tests/test_follow_tiers_cpu.py walks every plausible start of its images with both; tests/test_gpu_parity.py compares every
// quad and candidate with the oracle; tools/fuzz_parity.py sweeps).
constexpr unsigned LW_EXIT = 0x1c00u;        // exit direction << 10
constexpr unsigned LW_DELTA = 0x00030003u;   // (dx + 1) | (dy + 1) << 16

OCVAR_HD unsigned lean_table_entry(unsigned idx) {   // idx = t << 3 | first examined direction
    const unsigned from = idx & 7u, t = idx >> 3;
    const unsigned e = (from + t) & 7u;
    const unsigned dx = (unsigned)(step_dx((int)e) + 1), dy = (unsigned)(step_dy((int)e) + 1);
    // the t neighbours from, from + 1, ... were examined and found zero: was W (direction 4) / E (direction 0) among them?
    const unsigned pw = ((12u - from) & 7u) < t, pe = ((8u - from) & 7u) < t;
    return dx | (dy << 16) | (((e + 5u) & 7u) << 5) | (e << 10) | (pe << 30) | (pw << 31);
}

struct LeanWalk {
    unsigned xy;        // current pixel, x | y << 16
    unsigned m;         // its neighbour mask
    unsigned from;      // first direction examined from it = arrival direction + 1 (mod 8)
    unsigned pe;        // previous exit direction << 10: a corner point wherever the exit direction changes
    unsigned xy0, xy1;  // the border's first pixel and the pixel the closing step comes from
    unsigned cxy;       // the start's scan position as a packed point
    int npts, step, status;   // status: -1 while running, then a TraceStatus
};

OCVAR_HD void lean_begin(LeanWalk& w, const uint8_t* nbr, int ns, int cpos, int is_hole) {
    const int i0 = cpos - is_hole;
    const int x = i0 % ns, y = i0 / ns;
    w.xy = w.xy0 = (unsigned)x | ((unsigned)y << 16);
    w.cxy = w.xy0 + (unsigned)is_hole;   // (a hole's start position is the pixel east of its first pixel, same row)
    w.npts = 0;
    w.step = 0;
    w.status = -1;
    w.xy1 = 0;
    w.pe = 0;
    w.from = 0;
    w.m = nbr_of(nbr, x, y, ns);
    if (w.m == 0) {   // single-pixel domain (only reachable for outer borders)
        w.status = TRACE_SINGLE;
        w.npts = 1;
        return;
    }
    const int s = first_cw(w.m, (is_hole ? 0 : 4) - 1);   // direction of the border's last pixel seen from its first
    w.xy1 = w.xy0 + (unsigned)(step_dx(s) + 65536 * step_dy(s));
    w.pe = (unsigned)(s ^ 4) << 10;                        // prev_s = s ^ 4
    w.from = (unsigned)(s + 1) & 7u;
}

// One step of a running walk.  tab: the 64-entry table in LDS; base / nt / last: the walk's plane (its first byte, tiles per
// tile row = ns >> 4, the offset of its last 12-byte window); park(xy): the caller parks the pixel being left (every step; only a corner point
// advances npts afterwards).
template <class Park>
OCVAR_HD void lean_step(LeanWalk& w, const unsigned* tab, const uint8_t* base, unsigned nt, unsigned last, Park&& park) {
    const unsigned mm = byte_replicate(w.m);                       // the mask in all four bytes
    const unsigned t = (unsigned)__builtin_ctz(rotate_right(mm, w.from));   // zero neighbours before the next border pixel
    const unsigned ent = tab[(t << 3) + w.from];
    const int d = (int)(w.xy - w.cxy);                             // < 0: this pixel's west side precedes the start
    const unsigned nf = ((ent << 1) & (unsigned)(d + 1)) | (ent & (unsigned)d);   // sign: an earlier position of this border was passed
    const unsigned nxy = w.xy + (ent & LW_DELTA) - 0x10001u;
    const bool closes = (nxy == w.xy0) & (w.xy == w.xy1);
    const unsigned e = ent & LW_EXIT;
    const bool emit = e != w.pe;
    // the next pixel's 3x3 window in the bit plane (hd.h::nbr_win_off_xy on the packed point) and its mask (hd.h::nbr_mask9).  A
    // consistent plane never sends a walk outside itself; should one be inconsistent the offset is clamped (no access outside the
    // plane), the walk runs into its budget and the wave tier, which checks every coordinate, reports it.
    unsigned off = nbr_win_off_xy(nxy, nt);
    off = off < last ? off : last;
    const unsigned* win = reinterpret_cast<const unsigned*>(base + off);
    const unsigned m4 = nbr_mask9(win[0], win[1], win[2], nxy & 15u);
    park(w.xy);
    w.npts += emit ? 1 : 0;
    w.status = (int)nf < 0 ? (int)TRACE_NOT_FIRST : closes ? (int)TRACE_OK : m4 == 0u ? (int)TRACE_OVERRUN : -1;
    w.step += 1;
    w.xy = nxy;
    w.pe = e;
    w.from = (ent >> 5) & 7u;
    w.m = m4;
}

// The step budget of a tier-2 walk in an ROI of img_w x img_h pixels (frames: the batch's; crops: the one that fits the crop,
// croplist_core.h).  A walk whose step count has reached it ends as TRACE_OVERRUN; tier 2 compares once per block of steps, not in
// every step, so a walk may overshoot its budget by up to a block less one step.
template <bool CROP>
OCVAR_HD int lean_budget(int img_w, int img_h, int mid_steps, int budget) {
    return CROP ? crop_walk_budget(img_w & ~1, img_h & ~1, mid_steps, budget) : budget;
}

// ---- the window of the bit plane tier 3 walks in ------------------------------------------------------------------------------
// TILE_TX x TILE_TY tiles of the plane around the current pixel, copied to LDS by the wave.  In LDS the window is stored by
// column block: block i (columns tx0 + 16 i - 1 .. tx0 + 16 i + 16, a tile's 18 bits) holds the rows ty0 - 1 .. ty0 + TILE_H in
// TILE_SLOTS consecutive dwords, so a pixel's 3x3 window is dwords ly .. ly + 2 of its block -- no division by the tile height on
// the step's chain.  Dword d of window tile (i, j) is slot 14 j + d: a tile's apron rows land on the slots of the neighbouring
// tiles' rows, which they equal (follow_emul.cpp checks that on every load).
constexpr int TILE_TX = 4, TILE_TY = 5;    // the window in 16x14 tiles
constexpr int TILE_W = TILE_TX * NBR_TILE_W, TILE_H = TILE_TY * NBR_TILE_H;   // 64 x 70 pixels
constexpr int TILE_SLOTS = TILE_H + 2;
constexpr int TILE_QUARTERS = TILE_TX * TILE_TY * 4;   // a tile is loaded in quarters of 16 bytes (4 dwords)

// Origin of the window loaded for pixel (x, y) (tx0 a multiple of 16, ty0 of 14, either may be negative).  (bx, by): direction
// of travel; the window is pushed ahead so that a straight run re-centres as rarely as possible.
OCVAR_HD int tile_origin_x(int x, int bx) {
    return (x + 20 * bx - TILE_W / 2 + 8) & ~15;   // keeps x-20..x+27 inside for bx = 0, up to 55 pixels ahead otherwise
}
OCVAR_HD int tile_origin_y(int y, int by) {
    // rows: y - ty0 in [28, 42) for by = 0 (28 rows either side), [4, 18) going down, [52, 66) going up (ty0 a whole tile row;
    // the offset keeps the division's operand positive)
    return (int)div14((unsigned)(y + 24 * by - 28 + 4 * NBR_TILE_H)) * NBR_TILE_H - 4 * NBR_TILE_H;
}

// The window is loaded by quarter tiles of 16 bytes (4 dwords).  Quarter q (0 <= q < TILE_QUARTERS) is quarter q & 3 of window
// tile (i, j) = ((q >> 2) % TILE_TX, (q >> 2) / TILE_TX), which is tile (tx + i, ty + j) of the plane: (tx, ty) = the origin in
// tiles (tx0 >> 4, ty0 / 14).  A plane of ns columns and nty tile rows holds the tile when both tests below say so (the others
// are loaded as zeros); then its 16 bytes are at tile_quarter_src; its four dwords go to tile_quarter_dst in the window.
OCVAR_HD int tile_quarter_i(int q) { return (q >> 2) % TILE_TX; }
OCVAR_HD int tile_quarter_j(int q) { return (q >> 2) / TILE_TX; }
OCVAR_HD bool tile_quarter_col_in_plane(int q, int tx, int ns) {
    const int i = tile_quarter_i(q);
    return tx + i >= 0 && (tx + i) * 16 < ns;
}
OCVAR_HD bool tile_quarter_row_in_plane(int q, int ty, int nty) {
    const int j = tile_quarter_j(q);
    return ty + j >= 0 && ty + j < nty;
}
OCVAR_HD const uint8_t* tile_quarter_src(const uint8_t* plane, int q, int tx, int ty, int ns) {
    const int i = tile_quarter_i(q), j = tile_quarter_j(q);
    return plane + nbr_tile_off((unsigned)(tx + i), (unsigned)(ty + j), ns) + 16 * (q & 3);
}
OCVAR_HD unsigned* tile_quarter_dst(unsigned* win, int q) {
    const int i = tile_quarter_i(q), j = tile_quarter_j(q);
    return win + i * TILE_SLOTS + NBR_TILE_H * j + 4 * (q & 3);
}

// the pixel lies outside the window at (tx0, ty0)
OCVAR_HD bool tile_misses(int tx0, int ty0, int x, int y) {
    return (unsigned)(x - tx0) >= (unsigned)TILE_W || (unsigned)(y - ty0) >= (unsigned)TILE_H;
}

// mask of window pixel (lx, ly), 0 <= lx < TILE_W, 0 <= ly < TILE_H; win: the window's TILE_TX * TILE_SLOTS dwords
OCVAR_HD unsigned tile_mask(const unsigned* win, int lx, int ly) {
    const unsigned* w = win + ((unsigned)lx >> 4) * TILE_SLOTS + (unsigned)ly;
    return nbr_mask9(w[0], w[1], w[2], (unsigned)lx & 15u);
}

// Tier 3's step decode (the rules of trace_core.h::trace_border): from the pixel's mask m and the direction s the walk looks
// back in, the first direction examined, the zero neighbours passed before the next border pixel, the exit direction, and the
// passed neighbours as a mask (bit 4 = W, bit 0 = E).
struct TileStep {
    int from, tz, e;
    unsigned passed;
};
OCVAR_HD TileStep tile_step(unsigned m, int s) {
    TileStep d;
    d.from = (s + 1) & 7;
    d.tz = __builtin_ctz(((m * 0x101u) >> d.from) & 0xffu);
    d.e = (d.from + d.tz) & 7;
    d.passed = ((((1u << d.tz) - 1u) * 0x101u) << d.from) >> 8;
    return d;
}

}  // namespace ocvar

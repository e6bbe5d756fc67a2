// follow_emul.cpp -- host build of follower tiers 2 and 3 for tests/test_follow_tiers_cpu.py.  TEST ONLY: nothing in the
// product links this.  Built with -DOCVAR_NBR_TILED: everything here reads the product's bit plane.
//
// Tier 2 is walk_core.h's code itself: lean_begin, then lean_step from a 64-entry table filled by lean_table_entry, stepped in
// blocks with the budget looked at between blocks, as follow.hip::follow_mid_kernel does.  What the kernel adds -- parking the
// points in LDS, flushing them to slabs, the hand-out -- is not emulated; here `park` writes the point to an array.
//
// Tier 3 is a host emulation of the wave of follow.hip::trace_lean_tiled: the 64 lanes are a loop, LDS is an array, a ballot
// is "the first lane for which".  Its control flow is restated here (a form of the walker that exists once compiled to other
// device code); the arithmetic it evaluates is walk_core.h's, shared with the kernel: the window's constants, origin and
// quarter-tile mapping, tile_misses, tile_mask and tile_step.  The two "an earlier position of this border was passed" tests
// are restated as well.  tile_load makes three checks of its own (Tier3::err).
#include "walk_core.h"
#include "plane_writer.h"
#include <vector>

using namespace ocvar;

namespace {

constexpr int BLOCK = CROP_BUDGET_BLOCK;   // steps between two looks at the budget (follow.hip: MID_BLOCK, asserted equal there)

struct Plane {
    std::vector<uint8_t> bytes;
    int sw, sh, ns;
    Plane(const uint8_t* bin, int sw_, int sh_) : bytes((size_t)nbr_plane_bytes(emul_plane_ns(sw_), sh_)), sw(sw_), sh(sh_), ns(emul_plane_ns(sw_)) {
        emul_make_plane(bin, sw, sh, bytes.data());
    }
};

// ---- tier 2 ----
// pts: the corner points, packed x | y << 16 (room for every step of the walk + 1)
// marks: the corner points completed after every block of steps -- where follow_mid_kernel flushes a walk's parked points: a
// lane gets its start between two blocks, so a walk's blocks are counted from its own first step
LeanWalk tier2(const Plane& p, const unsigned* tab, int cpos, int is_hole, int budget, unsigned* pts, std::vector<int>* marks = nullptr) {
    LeanWalk w;
    lean_begin(w, p.bytes.data(), p.ns, cpos, is_hole);
    const unsigned nt = (unsigned)(p.ns >> 4), last = (unsigned)nbr_plane_bytes(p.ns, p.sh) - 12u;   // (as follow_mid_kernel's pl_nt, pl_last)
    while (w.status < 0) {
        for (int k = 0; k < BLOCK && w.status < 0; k++)
            lean_step(w, tab, p.bytes.data(), nt, last, [&](unsigned xy) { pts[w.npts] = xy; });   // (every step; only a corner point advances npts)
        if (w.status < 0 && w.step >= budget) w.status = TRACE_OVERRUN;
        if (marks) marks->push_back(w.npts);
    }
    return w;
}

// ---- tier 3 ----
enum { ERR_SLOT = 0, ERR_APRON = 1, ERR_READ = 2, ERR_SRC = 3, ERR_SPIN = 4, N_ERR = 5 };

struct Tier3 {
    unsigned lds[TILE_TX * TILE_SLOTS];
    const Plane* p;
    int tx0, ty0;
    long long loads;
    bool closed_in_run;
    // ERR_SLOT: a window slot written outside the array; ERR_APRON: two quarter tiles wrote different values to one slot;
    // ERR_READ: a mask read outside the loaded window; ERR_SRC: a plane read outside the plane; ERR_SPIN: the run loop went round without moving on
    long long err[N_ERR];
};

void tile_load(Tier3& t, int x, int y, int bx = 0, int by = 0) {
    t.tx0 = tile_origin_x(x, bx);
    t.ty0 = tile_origin_y(y, by);
    t.loads++;
    const int tx = (t.tx0 >> 4), ty = t.ty0 / NBR_TILE_H, nty = (t.p->sh + NBR_TILE_H - 1) / NBR_TILE_H;
    bool written[TILE_TX * TILE_SLOTS] = {};
    for (int h = 0; h < 2; h++)
        for (int lane = 0; lane < 64; lane++) {
            const int q = lane + 64 * h;
            if (q >= TILE_QUARTERS) continue;
            unsigned v[4] = {0u, 0u, 0u, 0u};
            if (tile_quarter_col_in_plane(q, tx, t.p->ns) && tile_quarter_row_in_plane(q, ty, nty)) {
                const uint8_t* src = tile_quarter_src(t.p->bytes.data(), q, tx, ty, t.p->ns);
                if (src < t.p->bytes.data() || src + 16 > t.p->bytes.data() + t.p->bytes.size()) {
                    t.err[ERR_SRC]++;
                } else {
                    for (int k = 0; k < 4; k++) v[k] = reinterpret_cast<const unsigned*>(src)[k];
                }
            }
            const long long slot = tile_quarter_dst(t.lds, q) - t.lds;
            for (int k = 0; k < 4; k++) {
                if (slot + k < 0 || slot + k >= TILE_TX * TILE_SLOTS) {
                    t.err[ERR_SLOT]++;
                    continue;
                }
                if (written[slot + k] && t.lds[slot + k] != v[k]) t.err[ERR_APRON]++;
                written[slot + k] = true;
                t.lds[slot + k] = v[k];
            }
        }
}

unsigned mask_at(Tier3& t, int x, int y) {   // tile_mask of plane pixel (x, y), which must lie in the loaded window
    const int lx = x - t.tx0, ly = y - t.ty0;
    if (lx < 0 || lx >= TILE_W || ly < 0 || ly >= TILE_H || t.loads == 0) {
        t.err[ERR_READ]++;
        return 0u;
    }
    return tile_mask(t.lds, lx, ly);
}

unsigned tile_get(Tier3& t, int x, int y) {
    if (tile_misses(t.tx0, t.ty0, x, y)) tile_load(t, x, y);
    return mask_at(t, x, y);
}

// follow.hip::trace_lean_tiled, statement for statement; out: packed points, 64 at a time from the lanes' hp
LeanTrace tier3(Tier3& t, int cpos, int is_hole, unsigned* out1, int max_pts, int max_steps) {
    LeanTrace r;
    r.status = TRACE_OK;
    r.npts = 0;
    r.steps = 0;
    const int ns = t.p->ns, sh = t.p->sh;
    const int i0 = cpos - is_hole;
    const int x0 = i0 % ns, y0 = i0 / ns;
    int x = x0, y = y0;
    unsigned m = tile_get(t, x, y);
    if (m == 0) {
        r.status = TRACE_SINGLE;
        r.npts = 1;
        return r;
    }
    int s = first_cw(m, (is_hole ? 0 : 4) - 1);
    const int x1 = x0 + step_dx(s), y1 = y0 + step_dy(s);
    int prev_s = s ^ 4;
    int straight = 0;
    int step = 0;
    unsigned hp[64] = {};
    for (;; step++) {
        if (step >= max_steps) {
            r.status = TRACE_OVERRUN;
            break;
        }
        const TileStep d = tile_step(m, s);
        const int e = d.e;
        const unsigned passed = d.passed;
        const int idx = y * ns + x;
        if (((passed & 0x10u) && idx < cpos) || ((passed & 1u) && idx + 1 < cpos)) {
            r.status = TRACE_NOT_FIRST;
            break;
        }
        if (e != prev_s) {
            if (r.npts < max_pts) {
                const int slot = r.npts & 63;
                hp[slot] = (unsigned)x | ((unsigned)y << 16);
                if (slot == 63)
                    for (int lane = 0; lane < 64; lane++) out1[r.npts - 63 + lane] = hp[lane];
            }
            r.npts++;
            prev_s = e;
        }
        const int ddx = step_dx(e), ddy = step_dy(e);
        const int px = x, py = y;
        x += ddx;
        y += ddy;
        if (x == x0 && y == y0 && px == x1 && py == y1) break;
        if ((unsigned)x >= (unsigned)ns || (unsigned)y >= (unsigned)sh) {
            r.status = TRACE_OVERRUN;
            break;
        }
        unsigned m4 = tile_get(t, x, y);
        if (m4 == 0) {
            r.status = TRACE_OVERRUN;
            break;
        }
        if (e == (s ^ 4) && m4 == m) {
            if (++straight >= 2) {
                bool closed = false, bad = false;
                for (int spin = 0;; spin++) {
                    // (emulation only, the kernel's loop has no such guard: a round jumps at least one pixel of the line or re-centres
                    // the window, and the round after a re-centring jumps)
                    if (spin > 2 * (ns + sh) + 16) {
                        t.err[ERR_SPIN]++;
                        r.status = TRACE_OVERRUN;
                        bad = true;
                        break;
                    }
                    // the ballots: the first lane whose pixel closes the border or carries another mask
                    int k = 64;
                    bool k_closes = false;
                    unsigned stop_m = 0;
                    for (int lane = 0; lane < 64; lane++) {
                        const int qx = x + (lane + 1) * ddx, qy = y + (lane + 1) * ddy;
                        const bool in_tile = (unsigned)(qx - t.tx0) < (unsigned)TILE_W && (unsigned)(qy - t.ty0) < (unsigned)TILE_H;
                        const unsigned mq = in_tile ? mask_at(t, qx, qy) : 256u;
                        const bool closes = qx == x0 && qy == y0 && qx - ddx == x1 && qy - ddy == y1;
                        if (closes || mq != m) {
                            k = lane;
                            k_closes = closes;
                            stop_m = mq;
                            break;
                        }
                    }
                    const int pa = y * ns + x, pb = (y + k * ddy) * ns + x + k * ddx;
                    if (((passed & 0x10u) && (pa < cpos || pb < cpos)) || ((passed & 1u) && (pa + 1 < cpos || pb + 1 < cpos))) {
                        r.status = TRACE_NOT_FIRST;
                        bad = true;
                        break;
                    }
                    x += k * ddx;
                    y += k * ddy;
                    step += k;
                    if (step >= max_steps) {
                        r.status = TRACE_OVERRUN;
                        bad = true;
                        break;
                    }
                    if (k == 64) continue;
                    if (k_closes) {
                        closed = true;
                        break;
                    }
                    if (stop_m == 256u) {
                        if ((unsigned)(x + ddx) >= (unsigned)ns || (unsigned)(y + ddy) >= (unsigned)sh) {
                            r.status = TRACE_OVERRUN;
                            bad = true;
                            break;
                        }
                        tile_load(t, x + ddx, y + ddy, ddx, ddy);
                        continue;
                    }
                    x += ddx;
                    y += ddy;
                    step++;
                    m4 = stop_m;
                    break;
                }
                if (closed) t.closed_in_run = true;
                if (bad || closed) break;
                if (m4 == 0) {
                    r.status = TRACE_OVERRUN;
                    break;
                }
                straight = 0;
            }
        } else {
            straight = 0;
        }
        m = m4;
        s = e ^ 4;
    }
    if (r.status == TRACE_OK) {
        const int stored = r.npts < max_pts ? r.npts : max_pts;
        const int rem = stored & 63;
        for (int lane = 0; lane < rem; lane++) out1[stored - rem + lane] = hp[lane];
    }
    r.steps = step;
    return r;
}

// the points of a closed border: n x,y pairs against n packed points
int same_points(const int* xy, const unsigned* packed, int n) {
    for (int i = 0; i < n; i++)
        if (packed[i] != ((unsigned)xy[2 * i] | ((unsigned)xy[2 * i + 1] << 16))) return 0;
    return 1;
}

// every stride-th plausible start of the image, in scan order
template <class F>
int for_each_start(const uint8_t* bin, int sw, int sh, int stride, int max_starts, F&& f) {
    const int ns = emul_plane_ns(sw);
    int n = 0, seen = 0;
    for (int y = 1; y < sh - 1; y++)
        for (int x = 1; x < sw - 1; x++) {
            const int c = emul_bin_at(bin, sw, sh, x, y), wv = emul_bin_at(bin, sw, sh, x - 1, y);
            if (c == wv) continue;   // neither an outer (0 -> 1) nor a hole (1 -> 0) start condition
            if (seen++ % stride != 0) continue;
            if (n >= max_starts) return -1;
            f(n++, y * ns + x, c ? 0 : 1);
        }
    return n;
}

}  // namespace

extern "C" int fe_row_ints() { return 24; }
extern "C" int fe_block() { return BLOCK; }
extern "C" int fe_window(int* out) {
    out[0] = TILE_TX; out[1] = TILE_TY; out[2] = TILE_W; out[3] = TILE_H; out[4] = TILE_SLOTS; out[5] = TILE_QUARTERS;
    return 6;
}
extern "C" int fe_lean_budget(int crop, int img_w, int img_h, int mid_steps, int budget) {
    return crop ? lean_budget<true>(img_w, img_h, mid_steps, budget) : lean_budget<false>(img_w, img_h, mid_steps, budget);
}

// Every plausible border start of the image (cvFindContours' outer / hole start conditions, enumerated as
// bitplane_emul.cpp::bp_walks does), walked four times on the same bit plane with the budget 4 ns sh + 16: trace_flat and
// tier 2, trace_border<true, false> and tier 3.  Per start fe_row_ints() ints:
//   0 cpos  1 is_hole
//   2 flat.status   3 flat.npts   4 flat.steps     5 tier2.status   6 tier2.npts   7 tier2.step    8 points equal (closed borders; else 1)
//   9 border.status 10 border.npts 11 border.steps 12 tier3.status 13 tier3.npts  14 tier3.steps  15 points equal (closed borders; else 1)
//  16 tier 3 closed the border inside a run   17 window loads   18.. the five error counts of Tier3::err
// stride: 1, or every stride-th start only (an image at the coordinate limit has 32 k starts of 65 k steps each).
// Returns the number of starts walked, -1 if there are more than max_starts.
extern "C" int fe_walks(const uint8_t* bin, int sw, int sh, int stride, int* rows, int max_starts) {
    const Plane p(bin, sw, sh);
    const int plane_pos = p.ns * sh, budget = 4 * p.ns * sh + 16;
    const int max_pts = budget;
    std::vector<int> ref(2 * ((size_t)max_pts + 1));
    std::vector<unsigned> got((size_t)max_pts + 64);
    unsigned tab[64];
    for (unsigned i = 0; i < 64; i++) tab[i] = lean_table_entry(i);
    return for_each_start(bin, sw, sh, stride, max_starts, [&](int n, int cpos, int hole) {
        int* o = rows + (size_t)fe_row_ints() * n;
        for (int i = 0; i < fe_row_ints(); i++) o[i] = 0;
        o[0] = cpos;
        o[1] = hole;
        const LeanTrace a = trace_flat(p.bytes.data(), p.ns, plane_pos, cpos, hole, ref.data(), max_pts, budget);
        const LeanWalk w = tier2(p, tab, cpos, hole, budget, got.data());
        o[2] = a.status; o[3] = a.npts; o[4] = a.steps;
        o[5] = w.status; o[6] = w.npts; o[7] = w.step;
        o[8] = (a.status == TRACE_OK && w.status == TRACE_OK && a.npts == w.npts) ? same_points(ref.data(), got.data(), a.npts) : 1;
        const TraceStats b = trace_border<true, false>(p.bytes.data(), p.ns, plane_pos, cpos, hole, ref.data(), max_pts, budget);
        Tier3 t = {};
        t.p = &p;
        t.tx0 = t.ty0 = -(1 << 28);   // (as follow_long_kernel: no window yet)
        const LeanTrace c = tier3(t, cpos, hole, got.data(), max_pts, budget);
        o[9] = b.status; o[10] = b.npts; o[11] = b.steps;
        o[12] = c.status; o[13] = c.npts; o[14] = c.steps;
        o[15] = (b.status == TRACE_OK && c.status == TRACE_OK && b.npts == c.npts) ? same_points(ref.data(), got.data(), b.npts) : 1;
        o[16] = t.closed_in_run ? 1 : 0;
        o[17] = (int)t.loads;
        for (int i = 0; i < N_ERR; i++) o[18 + i] = (int)t.err[i];
    });
}

// One start (cpos at the bit plane's pitch) walked by tier 2 with the budget 4 ns sh + 16: out[i] = corner points completed
// after block i of fe_block() steps, the last entry the border's point count.  Returns the number of blocks; -1 if the walk
// does not close or needs more than max_out blocks.
extern "C" int fe_tier2_marks(const uint8_t* bin, int sw, int sh, int cpos, int is_hole, int* out, int max_out) {
    const Plane p(bin, sw, sh);
    const int budget = 4 * p.ns * sh + 16;
    std::vector<unsigned> got((size_t)budget + BLOCK + 64);
    std::vector<int> marks;
    unsigned tab[64];
    for (unsigned i = 0; i < 64; i++) tab[i] = lean_table_entry(i);
    const LeanWalk w = tier2(p, tab, cpos, is_hole, budget, got.data(), &marks);
    if (w.status != TRACE_OK || (int)marks.size() > max_out) return -1;
    for (size_t i = 0; i < marks.size(); i++) out[i] = marks[i];
    return (int)marks.size();
}

// Every plausible start with a step budget: tier 2 as the kernel ends it (the budget looked at after every block of fe_block()
// steps) against trace_flat with max_steps.  Per start 8 ints: cpos, is_hole, flat status / npts / steps, tier 2 status / npts / step.
extern "C" int fe_budget_walks(const uint8_t* bin, int sw, int sh, int budget, int flat_max_steps, int* rows, int max_starts) {
    const Plane p(bin, sw, sh);
    std::vector<unsigned> got((size_t)budget + BLOCK + 64);
    unsigned tab[64];
    for (unsigned i = 0; i < 64; i++) tab[i] = lean_table_entry(i);
    return for_each_start(bin, sw, sh, 1, max_starts, [&](int n, int cpos, int hole) {
        int* o = rows + 8 * (size_t)n;
        const LeanTrace a = trace_flat(p.bytes.data(), p.ns, p.ns * sh, cpos, hole, nullptr, 0, flat_max_steps);
        const LeanWalk w = tier2(p, tab, cpos, hole, budget, got.data());
        o[0] = cpos; o[1] = hole;
        o[2] = a.status; o[3] = a.npts; o[4] = a.steps;
        o[5] = w.status; o[6] = w.npts; o[7] = w.step;
    });
}

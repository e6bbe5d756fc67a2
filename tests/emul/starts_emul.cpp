// starts_emul.cpp -- host build of starts_core.h for tests/test_starts_cpu.py.  TEST ONLY.
// se_rule is the border-start rule spelt out pixel by pixel; se_pairs and se_walk run the word-parallel core of the binarise
// kernels against it: on single row pairs, and on whole binary images walked as binarise.hip::march_unit walks them -- work
// units of whole tile rows, strips of 240 columns, 15 tiles per strip, four lanes per tile with four rows each, the row above a
// lane's first row taken from the lane before it.  Bits of a lane's words that the kernel does not compute reliably (the halo
// columns beyond a strip's two apron columns) are filled with noise here: the core's masks must keep them out of the result.
#include <cstdint>
#include "starts_core.h"

using namespace ocvar;

namespace {

constexpr int STRIP = 240;   // kernels.h::MARCH_STRIP (kernels.h itself needs the HIP runtime)

struct Img {
    const uint8_t* b;
    int sw, sh;
    unsigned at(int x, int y) const { return x >= 0 && x < sw && y >= 0 && y < sh && b[(long long)y * sw + x] ? 1u : 0u; }
};

// the rule of starts_core.h for one pixel: 1 an outer start, 2 a hole start, 0 neither
int rule_at(const Img& im, int x, int y) {
    const unsigned c = im.at(x, y), W = im.at(x - 1, y), E = im.at(x + 1, y);
    const unsigned NW = im.at(x - 1, y - 1), N = im.at(x, y - 1), NE = im.at(x + 1, y - 1);
    const unsigned NEE = x % STRIP == STRIP - 1 ? 0u : im.at(x + 2, y - 1);   // (not computed at a strip's last column)
    if (c && !W && !NW && !N && !NE && !(E && NEE)) return 1;
    if (!c && W && N && (E || NE)) return 2;
    return 0;
}

struct Rng {
    uint64_t s;
    unsigned next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)(s >> 33);
    }
};

}  // namespace

extern "C" {

// every start of the image, as y * sw + x with the hole flag in bit 31; returns the count (entries beyond cap are not written)
int se_rule(const uint8_t* b, int sw, int sh, unsigned* out, int cap) {
    const Img im{b, sw, sh};
    int n = 0;
    for (int y = 0; y < sh; y++)
        for (int x = 0; x < sw; x++) {
            const int k = rule_at(im, x, y);
            if (!k) continue;
            if (n < cap) out[n] = (unsigned)(y * sw + x) | (k == 2 ? 0x80000000u : 0u);
            n++;
        }
    return n;
}

// n row pairs (c: the row, a: the row above; bit k = column k): bits 1 .. 29 of the core's words against the rule, pixel by
// pixel (bit 0 and bits 30, 31 read neighbours outside the word) -- the two word functions, and starts_of_lane's own spelling of
// them (a lane whose second row is the pair's row, on its own columns).  Returns the number of differing bits.
long long se_pairs(const unsigned* c, const unsigned* a, int n) {
    long long bad = 0;
    for (int i = 0; i < n; i++) {
        const unsigned o = starts_outer(c[i], a[i]), h = starts_hole(c[i], a[i]);
        const unsigned w[4] = {a[i], c[i], 0u, 0u};
        unsigned long long any, hole;
        starts_of_lane(w, 0u, 3, NBR_TILE_H, STARTS_OWN_BITS, any, hole);   // (the own columns of the lane's second row: bits 16 .. 31)
        const unsigned lane_any = ((unsigned)any >> 16) << STARTS_WORD_LEAD, lane_hole = ((unsigned)hole >> 16) << STARTS_WORD_LEAD;
        bad += __builtin_popcount((lane_any ^ (o | h)) & STARTS_OWN_BITS) + __builtin_popcount((lane_hole ^ h) & STARTS_OWN_BITS);
        for (int k = 1; k <= 29; k++) {
            auto bit = [](unsigned v, int j) { return (v >> j) & 1u; };
            const unsigned C = bit(c[i], k), W = bit(c[i], k - 1), E = bit(c[i], k + 1);
            const unsigned NW = bit(a[i], k - 1), N = bit(a[i], k), NE = bit(a[i], k + 1), NEE = bit(a[i], k + 2);
            const unsigned ro = C && !W && !NW && !N && !NE && !(E && NEE), rh = !C && W && N && (E || NE);
            bad += (bit(o, k) != ro) + (bit(h, k) != rh);
        }
    }
    return bad;
}

// the starts of the image found as the kernel finds them, cut into work units of unit_rows rows (a multiple of 14)
int se_walk(const uint8_t* b, int sw, int sh, int unit_rows, unsigned seed, unsigned* out, int cap) {
    const Img im{b, sw, sh};
    Rng rng{seed * 2654435761ull + 1};
    int n = 0;
    if (unit_rows < NBR_TILE_H || unit_rows % NBR_TILE_H) return -1;
    for (int Y0 = 0; Y0 < sh; Y0 += unit_rows) {
        const int Y1 = Y0 + unit_rows < sh ? Y0 + unit_rows : sh;
        for (int strip = 0; strip * STRIP < sw; strip++)
            for (int ty = Y0 / NBR_TILE_H; ty < (Y1 + NBR_TILE_H - 1) / NBR_TILE_H; ty++) {
                const int nrows = Y1 - NBR_TILE_H * ty < NBR_TILE_H ? Y1 - NBR_TILE_H * ty : NBR_TILE_H;
                for (int tx = 0; tx < STARTS_STRIP_TILES; tx++) {
                    const int col0 = strip * STRIP + NBR_TILE_W * tx;
                    unsigned prev3 = rng.next();   // (q = 0 has no lane before it in the quad: whatever the shift brings)
                    for (int q = 0; q < 4; q++) {
                        unsigned w[4];
                        for (int i = 0; i < 4; i++) {
                            const int r = NBR_TILE_H * ty + 4 * q + i - 1;
                            unsigned ww = 0;
                            for (int k = 0; k < 32; k++) {
                                const int sc = NBR_TILE_W * tx - STARTS_WORD_LEAD + k;   // column within the strip
                                // rows Y0 - 1 .. Y1 of columns -1 .. 240 of the strip are what the wave computed (0 outside the image)
                                // -- everything else in the ring is noise: other columns of the halo lanes, stale rows
                                const unsigned bit = sc >= -1 && sc <= STRIP && r >= Y0 - 1 && r <= Y1 ? im.at(strip * STRIP + sc, r) : rng.next() & 1u;
                                ww |= bit << k;
                            }
                            w[i] = (unsigned)r <= (unsigned)Y1 ? ww & starts_word_bits(tx) : 0u;
                        }
                        unsigned long long any, hole;
                        starts_of_lane(w, prev3, 4 * q - 1, nrows, starts_own_bits(col0, sw), any, hole);
                        prev3 = w[3];
                        for (int k = 0; k < 64; k++) {
                            if (!((any >> k) & 1ull)) continue;
                            const int y = NBR_TILE_H * ty + 4 * q - 1 + (k >> 4), x = col0 + (k & 15);
                            if (n < cap) out[n] = (unsigned)(y * sw + x) | (unsigned)((hole >> k) & 1ull) << 31;
                            n++;
                        }
                    }
                }
            }
    }
    return n;
}

}  // extern "C"

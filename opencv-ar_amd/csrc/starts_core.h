// starts_core.h -- where a border can begin, found on whole words of threshold bits, free of HIP calls.
// binarise.hip::march_unit calls starts_of_lane when it has the rows of a tile row of the bit plane in hand (flush_tiles);
// tests/emul/starts_emul.cpp builds the same functions for the host and walks random binary images tile row by tile row as the
// kernel does (tests/test_starts_cpu.py, against the per-pixel rule).
//
// The rule (necessary local conditions for being the raster-first pixel of a region; the followers decide the rest):
//   outer start: a foreground pixel whose W, NW, N and NE are background -- and not (E foreground and the pixel above E's east
//                neighbour foreground: that one belongs to the same 8-connected component and comes earlier);
//   hole start:  a background pixel whose W and N are foreground -- and E or NE foreground (if both are background the pixel and
//                NE belong to the same 4-connected background region and NE comes earlier).
// With c a row's bits and a the bits of the row above, bit k = column k, every neighbour is a shift: W = c << 1, E = c >> 1,
// NW = a << 1, N = a, NE = a >> 1, the pixel above E's east neighbour a >> 2.  A bit of the result is right where the bits it
// reads are: a word's lowest bit and its two highest see neighbours the word does not hold.
#pragma once
#include "hd.h"

namespace ocvar {

OCVAR_HD unsigned starts_outer(unsigned c, unsigned a) { return c & ~(c << 1) & ~((a << 1) | a | (a >> 1)) & ~((c >> 1) & (a >> 2)); }
OCVAR_HD unsigned starts_hole(unsigned c, unsigned a) { return (c << 1) & ~c & a & ((c >> 1) | (a >> 1)); }

// ---- a lane's share of a tile row ------------------------------------------------------------------------------------------------
// When tile row ty of a strip is flushed, lane l (< 60) holds four row words of tile tx = l >> 2: rows 14 ty + 4 q - 1 + i
// (q = l & 3, i = 0 .. 3), bit k = column 16 tx - 8 + k of the strip.  The tile's own pixels are columns 16 tx .. 16 tx + 15
// (bits 8 .. 23) of rows 14 ty .. 14 ty + 13: the first word of q = 0 is the tile's apron row (the row above its first row), the
// last word of q = 3 the apron row below; a start test of bits 8 .. 23 reads bits 7 .. 25.
constexpr int STARTS_WORD_LEAD = 8;                 // columns of a lane's word before its tile's first column
constexpr unsigned STARTS_OWN_BITS = 0x00ffff00u;   // the tile's own columns in a lane's word
constexpr int STARTS_STRIP_TILES = 15;              // tiles of a strip's tile row (240 columns)

// Bits of a lane's row words that hold threshold bits at all.  A strip's wave computes its 240 columns and one more on each side
// (the apron columns -1 and 240); column 241 -- bit 25 of the strip's last tile, which only "the pixel above E's east neighbour"
// of column 239 reads -- is not computed and counts as background: at the last column of a strip that exclusion is not applied
// (a few more plausible starts, which the followers discard).
OCVAR_HD unsigned starts_word_bits(int tile_in_strip) { return tile_in_strip == STARTS_STRIP_TILES - 1 ? ~(1u << 25) : ~0u; }

// Bits of a lane's word whose pixels may yield starts: the tile's own columns inside the image (col0: the tile's first column).
OCVAR_HD unsigned starts_own_bits(int col0, int sw) {
    const int n = sw - col0;
    return n <= 0 ? 0u : n >= NBR_TILE_W ? STARTS_OWN_BITS : ((1u << n) - 1u) << STARTS_WORD_LEAD;
}

// the own columns (bits 8 .. 23; the other bits are 0) of two rows' words in one word: the first row's in the low half
OCVAR_HD unsigned starts_pack2(unsigned lo, unsigned hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x06050201u);
#else
    return (lo >> STARTS_WORD_LEAD) | (hi << (16 - STARTS_WORD_LEAD));
#endif
}

// The starts of one lane's four rows.  w: the row words, already zero for rows that are not in the ring (rows outside [0, Y1])
// and masked with starts_word_bits; above: the word of the row before w[0] (the quad neighbour's w[3]; not read for q = 0, whose
// w[0] is the apron row); qrow = 4 q - 1: w[0]'s row within the tile row; nrows: the tile row's rows that belong to the unit,
// min(14, Y1 - 14 ty) -- a start row belongs to exactly one unit, its row above may be the unit's apron row Y0 - 1; own:
// starts_own_bits.  any / hole: bit 16 i + k = column 16 tx + k of row i is a start / a hole start.
//
// starts_outer and starts_hole are spelt out here with the shifts shared: a row's a is the row before's c, so a << 1, a >> 1 and
// a >> 2 are that row's c << 1, c >> 1 and c >> 2 -- a row costs three new shifts (two for the last), the first row takes its
// three from above; and the logic is five operations of three inputs each, the form the device has an instruction for, and two
// more for sel.  (Written as calls of the two one-line functions, each row's five shifts were computed anew and in merged forms
// -- (a | c) >> 1 -- that nothing could share: 14 vector instructions per row where 10 do.)  Every shifted word below has more
// than one use, which is also what keeps a compiler from merging them again.  tests/test_starts_words_cpu.py holds this
// against the two functions row by row.
OCVAR_HD void starts_of_lane(const unsigned w[4], unsigned above, int qrow, int nrows, unsigned own, unsigned long long& any, unsigned long long& hole) {
    unsigned m[4], h[4];
    unsigned a = above, al = above << 1, ar = above >> 1, ar2 = above >> 2;
    OCVAR_UNROLL
    for (int i = 0; i < 4; i++) {
        const unsigned c = w[i], cl = c << 1, cr = c >> 1;
        const unsigned sel = (unsigned)(qrow + i) < (unsigned)nrows ? own : 0u;
        const unsigned n = al | a | ar;                 // NW, N or NE set
        const unsigned o1 = c & ~cl & ~n;
        const unsigned out = o1 & ~(cr & ar2);          // starts_outer(c, a)
        const unsigned h1 = cl & ~c & a;
        unsigned hs = h1 & (cr | ar);                   // starts_hole(c, a)
        OCVAR_OPAQUE(hs);                               // (else both uses below get a chain of their own from h1 on: two more per row)
        h[i] = hs & sel;
        m[i] = (out | hs) & sel;
        a = c;
        al = cl;
        ar = cr;
        if (i < 3) ar2 = c >> 2;
    }
    any = (unsigned long long)starts_pack2(m[0], m[1]) | ((unsigned long long)starts_pack2(m[2], m[3]) << 32);
    hole = (unsigned long long)starts_pack2(h[0], h[1]) | ((unsigned long long)starts_pack2(h[2], h[3]) << 32);
}

}  // namespace ocvar

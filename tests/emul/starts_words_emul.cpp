// starts_words_emul.cpp -- host build of starts_core.h::starts_of_lane for tests/test_starts_words_cpu.py.  TEST ONLY.
// sw_lanes calls starts_of_lane on n lanes' words as they are; sw_rows computes what it must give from the two one-line
// functions of the rule, starts_outer and starts_hole, applied row by row.  The Python test compares the two (and holds a
// transcription of the two formulas in numpy against sw_rows).
#include <cstdint>
#include "starts_core.h"

using namespace ocvar;

extern "C" {

// w: n x 4 row words, above: n words; any / hole: n 64-bit results each
void sw_lanes(const unsigned* w, const unsigned* above, int n, int qrow, int nrows, unsigned own, unsigned long long* any, unsigned long long* hole) {
    for (int i = 0; i < n; i++) starts_of_lane(w + 4 * i, above[i], qrow, nrows, own, any[i], hole[i]);
}

void sw_rows(const unsigned* w, const unsigned* above, int n, int qrow, int nrows, unsigned own, unsigned long long* any, unsigned long long* hole) {
    for (int i = 0; i < n; i++) {
        unsigned long long m = 0, h = 0;
        for (int r = 0; r < 4; r++) {
            const unsigned c = w[4 * i + r], a = r == 0 ? above[i] : w[4 * i + r - 1];
            const unsigned sel = qrow + r >= 0 && qrow + r < nrows ? own : 0u;
            const unsigned ho = starts_hole(c, a) & sel, ou = starts_outer(c, a) & sel;
            // bit 16 r + k of the result: column k of the tile = bit STARTS_WORD_LEAD + k of the row's word
            m |= (unsigned long long)(((ou | ho) >> STARTS_WORD_LEAD) & 0xffffu) << (16 * r);
            h |= (unsigned long long)((ho >> STARTS_WORD_LEAD) & 0xffffu) << (16 * r);
        }
        any[i] = m;
        hole[i] = h;
    }
}

unsigned sw_own_bits(int col0, int sw) { return starts_own_bits(col0, sw); }

}  // extern "C"

"""CPU test of starts_core.h::starts_of_lane on words: the function spells the border-start rule out with shared shifts and
three-input operations, and must give for every input what the two one-line functions of the rule, starts_outer and
starts_hole, give row by row -- on random words, on the all-ones and all-zeros words, and on single bits at the positions where
a word's own columns begin and end (7, 8, 23, 24, 25) and at the word's ends (0, 31); for the four places a lane has in its
tile (qrow = -1, 3, 7, 11) and tile rows of 1, 13 and 14 rows that belong to the unit.  tests/emul/starts_words_emul.cpp builds
both for the host."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers import P
from hostbuild import host_core

QROWS, NROWS = (-1, 3, 7, 11), (1, 13, 14)
OWN_ALL = 0x00FFFF00
SINGLE_BITS = (0, 7, 8, 23, 24, 25, 31)


def build_lib():
    l = host_core("starts_words_emul")
    for f in (l.sw_lanes, l.sw_rows):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
        f.restype = None
    l.sw_own_bits.restype = C.c_uint
    return l


@pytest.fixture(scope="module")
def lib():
    return build_lib()


def owns(lib):
    """every tile's own columns; a tile the image's right edge cuts to 5 columns and to 1; a tile outside the image"""
    got = [lib.sw_own_bits(0, 640), lib.sw_own_bits(16, 21), lib.sw_own_bits(32, 33), lib.sw_own_bits(48, 40)]
    assert got == [OWN_ALL, 0x00001F00, 0x00000100, 0]
    return got


def numpy_rows(w, above, qrow, nrows, own):
    """the two formulas of starts_core.h transcribed: outer = c & ~(c << 1) & ~((a << 1) | a | (a >> 1)) & ~((c >> 1) & (a >> 2)),
    hole = (c << 1) & ~c & a & ((c >> 1) | (a >> 1)), on 32-bit words"""
    M = np.uint64(0xFFFFFFFF)
    any_, hole = np.zeros(len(w), np.uint64), np.zeros(len(w), np.uint64)
    for r in range(4):
        c = w[:, r].astype(np.uint64)
        a = (above if r == 0 else w[:, r - 1]).astype(np.uint64)
        one, two = np.uint64(1), np.uint64(2)
        outer = c & ~((c << one) & M) & ~(((a << one) & M) | a | (a >> one)) & ~((c >> one) & (a >> two)) & M
        ho = ((c << one) & M) & ~c & a & ((c >> one) | (a >> one)) & M
        sel = np.uint64(own if 0 <= qrow + r < nrows else 0)
        ho, outer = ho & sel, outer & sel
        any_ |= (((outer | ho) >> np.uint64(8)) & np.uint64(0xFFFF)) << np.uint64(16 * r)
        hole |= ((ho >> np.uint64(8)) & np.uint64(0xFFFF)) << np.uint64(16 * r)
    return any_, hole


def check(lib, w, above, where):
    w = np.ascontiguousarray(w, np.uint32)
    above = np.ascontiguousarray(above, np.uint32)
    n = len(above)
    assert w.shape == (n, 4)
    starts = 0
    for qrow, nrows, own in itertools.product(QROWS, NROWS, owns(lib)):
        got_any, got_hole = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        ref_any, ref_hole = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        lib.sw_lanes(P(w), P(above), n, qrow, nrows, own, P(got_any), P(got_hole))
        lib.sw_rows(P(w), P(above), n, qrow, nrows, own, P(ref_any), P(ref_hole))
        np_any, np_hole = numpy_rows(w, above, qrow, nrows, own)
        assert (ref_any == np_any).all() and (ref_hole == np_hole).all(), (where, qrow, nrows, hex(own))
        bad = np.flatnonzero((got_any != ref_any) | (got_hole != ref_hole))
        assert len(bad) == 0, (where, qrow, nrows, hex(own), [hex(int(v)) for v in w[bad[0]]], hex(int(above[bad[0]])),
                               hex(int(got_any[bad[0]])), hex(int(ref_any[bad[0]])), hex(int(got_hole[bad[0]])), hex(int(ref_hole[bad[0]])))
        assert ((got_hole & ~got_any) == 0).all()   # a hole start is a start
        starts += int(np.unpackbits(got_any.view(np.uint8)).sum())
    return starts


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_random_words(lib, density):
    rng = np.random.default_rng(40 + int(density * 10))
    n = 20000
    bits = rng.random((n, 5, 32)) < density
    words = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    assert check(lib, words[:, :4], words[:, 4], ("random", density)) > 100   # (the comparison is of words that hold starts)


def test_ones_zeros_and_single_bits(lib):
    special = [0, 0xFFFFFFFF] + [1 << b for b in SINGLE_BITS]
    # every special word in every row with every special word above it, the other rows all zeros / all ones / the word again
    rows = []
    for s, t in itertools.product(special, special):
        for r in range(4):
            for fill in (0, 0xFFFFFFFF, s):
                w = [fill] * 4
                w[r] = s
                rows.append(w + [t])
    # and every quadruple of {zeros, ones, a single bit} with each of them above
    few = [0, 0xFFFFFFFF, 1 << 8, 1 << 23]
    rows += [list(q) for q in itertools.product(few, repeat=5)]
    a = np.array(rows, np.uint64).astype(np.uint32)
    assert check(lib, a[:, :4], a[:, 4], "special") > 0


def test_neighbouring_single_bits(lib):
    """a start's neighbours one and two columns away, across the ends of the own columns: pairs of single-bit words in
    consecutive rows at every pair of positions d apart, |d| <= 2, around the positions of the list"""
    rows = []
    for b in SINGLE_BITS:
        for d in (-2, -1, 0, 1, 2):
            if not 0 <= b + d <= 31:
                continue
            for r in range(4):
                w = [0, 0, 0, 0, 0]   # (index 4: above)
                w[r] = 1 << b
                w[r - 1 if r else 4] = 1 << (b + d)
                rows.append(w)
                rows.append([v | (1 << b) for v in w])   # and with the column of bit b set in all rows
    a = np.array(rows, np.uint64).astype(np.uint32)
    assert check(lib, a[:, :4], a[:, 4], "neighbours") > 0

"""CPU tests of starts_core.h, the word-parallel border-start test the binarise kernels run when they flush a tile row of the bit
plane.  tests/emul/starts_emul.cpp builds the core for the host next to the rule spelt out pixel by pixel: the two are compared
on random row pairs, and on whole binary images walked as the kernel walks them (work units of whole tile rows, 240-column
strips, four lanes per 16x14 tile), where the words' unreliable bits -- halo columns, stale ring rows -- are noise."""
import ctypes as C

import numpy as np
import pytest

from helpers import P
from hostbuild import host_core


def build_lib():
    l = host_core("starts_emul")
    l.se_pairs.restype = C.c_longlong
    l.se_walk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int]
    return l


@pytest.fixture(scope="module")
def lib():
    return build_lib()


def _rule(lib, b):
    sh, sw = b.shape
    out = np.zeros(b.size + 1, np.uint32)
    n = lib.se_rule(P(b), sw, sh, P(out), out.size)
    assert 0 <= n <= out.size
    return np.sort(out[:n])


def _walk(lib, b, unit_rows, seed):
    sh, sw = b.shape
    out = np.zeros(b.size + 1, np.uint32)
    n = lib.se_walk(P(b), sw, sh, unit_rows, seed, P(out), out.size)
    assert 0 <= n <= out.size
    return np.sort(out[:n])


def _framed(b):
    """cvFindContours' zeroed one-pixel frame, as the kernels' threshold rows have it"""
    b = np.ascontiguousarray(b.astype(np.uint8))
    b[0, :] = b[-1, :] = 0
    b[:, 0] = b[:, -1] = 0
    return b


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_core_equals_the_pixel_rule_on_row_pairs(lib, density):
    rng = np.random.default_rng(int(density * 10))
    n = 20000
    bits = rng.random((2, n, 32)) < density
    words = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    c, a = np.ascontiguousarray(words[0]), np.ascontiguousarray(words[1])
    assert lib.se_pairs(P(c), P(a), n) == 0


# widths: word and tile edges (31, 32), a whole strip and its last column's exception (240), a second strip of one column and of
# ten (241, 250); heights: partial tile rows (13, 14, 15) and the unit boundary at row 252 (260)
SHAPES = [(h, w) for w in (31, 32, 240, 241, 250) for h in (13, 14, 15, 260)]


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_walk_by_tile_rows_finds_the_rule_s_starts(lib, density):
    rng = np.random.default_rng(11 + int(density * 10))
    total = 0
    for h, w in SHAPES:
        b = _framed(rng.random((h, w)) < density)
        ref = _rule(lib, b)
        for unit_rows in (252, 14, 42):   # the crop pass's units, and cuts a frame's chunks can have
            got = _walk(lib, b, unit_rows, seed=h * 1000 + w)
            assert got.shape == ref.shape and (got == ref).all(), (h, w, unit_rows)
        total += len(ref)
    assert total > 1000


def test_starts_do_not_depend_on_the_noise_or_the_cut(lib):
    b = _framed(np.random.default_rng(5).random((260, 250)) < 0.5)
    ref = _walk(lib, b, 252, seed=1)
    for unit_rows, seed in ((252, 2), (14, 3), (28, 4), (266, 5)):
        assert (_walk(lib, b, unit_rows, seed) == ref).all()
    assert lib.se_walk(P(b), 250, 260, 15, 0, None, 0) == -1   # (units are whole tile rows)


def test_last_column_of_a_strip_keeps_its_exception(lib):
    # pixel (239, 2) with E and the pixel above E's east neighbour set: excluded anywhere else, a start at a strip's last column
    b = np.zeros((6, 250), np.uint8)
    b[2, 239] = b[2, 240] = b[1, 241] = 1
    c = np.zeros((6, 250), np.uint8)
    c[2, 100] = c[2, 101] = c[1, 102] = 1
    for img, x, want in ((b, 239, True), (c, 100, False)):
        ref, got = _rule(lib, img), _walk(lib, img, 252, seed=9)
        assert (ref == got).all()
        assert ((2 * 250 + x) in set(got.tolist())) == want


def test_zeroed_frame_and_solid_images(lib):
    for h, w in ((13, 31), (15, 241), (260, 32)):
        solid = _framed(np.ones((h, w)))   # one region: its first pixel is the only start
        got = _walk(lib, solid, 252, seed=3)
        assert got.tolist() == [1 * w + 1] and (got == _rule(lib, solid)).all()
        ring = solid.copy()
        ring[3:-3, 3:-3] = 0   # a hole: one more start, flagged
        got = _walk(lib, ring, 252, seed=4)
        assert (got == _rule(lib, ring)).all() and got.tolist() == [1 * w + 1, (3 * w + 3) | 0x80000000]
        assert len(_walk(lib, np.zeros((h, w), np.uint8), 252, seed=5)) == 0

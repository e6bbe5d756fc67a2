"""CPU tests of the frame-block rules every frame operation shares (opencv-ar_amd/csrc/frames_core.h, built for the host from
tests/emul/frames_emul.cpp): bytes per pixel, row span, extent, intersection, the one check and the dword predicate, held to
the same rules stated here in Python's unbounded integers -- at the edges where 64-bit arithmetic or an off-by-one could slip."""
import ctypes as C
import itertools
import os
import re

import pytest

import helpers as H
from hostbuild import host_core

OK, FORMAT, SIDE, COUNT, ROW_STRIDE, SPAN = range(6)     # frames_core.h: FramesBad
MAX_SPAN = 2147483647
ANY = 32767                                               # the side limit of resize, orient, warp and levels
CONTEXT = (640, 480)                                      # a context's size, the other kind of limit
BASE = 1 << 40                                            # a first byte


class Block(C.Structure):
    _fields_ = [("p", C.c_ulonglong), ("width", C.c_int), ("height", C.c_int), ("bpp", C.c_int), ("row_stride", C.c_longlong),
                ("frame_stride", C.c_ulonglong), ("n_frames", C.c_int)]


def block(width, height, bpp, row_stride, frame_stride=0, n_frames=1, p=BASE):
    return Block(p, width, height, bpp, row_stride, frame_stride, n_frames)


@pytest.fixture(scope="module")
def lib():
    L = host_core("frames_emul")
    B = C.POINTER(Block)
    for name, res, args in (("bpp", C.c_int, [C.c_int]), ("row_span", C.c_longlong, [B]), ("extent", C.c_ulonglong, [B]),
                            ("intersect", C.c_int, [B, B]), ("check", C.c_int, [B, C.c_int, C.c_int]),
                            ("dwords", C.c_int, [C.c_ulonglong, C.c_longlong, C.c_longlong])):
        f = getattr(L, "frames_emul_" + name)
        f.restype, f.argtypes = res, args
    return L


# the rules, stated independently
def span_of(b):
    return (b.height - 1) * b.row_stride + b.bpp * b.width


def extent_of(b):
    return (b.n_frames - 1) * b.frame_stride + span_of(b)


def check_of(b, max_w, max_h):
    if b.bpp < 1:
        return FORMAT
    if not (1 <= b.width <= max_w and 1 <= b.height <= max_h):
        return SIDE
    if b.n_frames < 1:
        return COUNT
    if b.row_stride < b.bpp * b.width:
        return ROW_STRIDE
    return SPAN if span_of(b) > MAX_SPAN else OK


def intersect_of(a, b):
    return a.p < b.p + extent_of(b) and b.p < a.p + extent_of(a)


def agree(lib, b, max_w=ANY, max_h=ANY):
    got = lib.frames_emul_check(C.byref(b), max_w, max_h)
    assert got == check_of(b, max_w, max_h), (b.width, b.height, b.bpp, b.row_stride, b.n_frames, got)
    if got in (OK, SPAN):
        assert lib.frames_emul_row_span(C.byref(b)) == span_of(b)
    return got


def test_format_bpp_is_the_headers_table(lib):
    text = open(os.path.join(H.ROOT, "include", "ocvar_hip.h")).read()
    codes = {name: int(v) for name, v in re.findall(r"OCVAR_FMT_(\w+) = (\d+)", text)}
    assert codes == {"BGR": 0, "RGB": 1, "BGRA": 2, "RGBA": 3, "GRAY": 4}
    want = {codes["BGR"]: 3, codes["RGB"]: 3, codes["BGRA"]: 4, codes["RGBA"]: 4, codes["GRAY"]: 1}
    for fmt in range(-2, 8):
        assert lib.frames_emul_bpp(fmt) == want.get(fmt, 0), fmt
    b = block(4, 4, lib.frames_emul_bpp(7), 16)
    assert agree(lib, b) == FORMAT


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_row_stride_edge(lib, bpp):
    for width in (1, ANY):
        assert agree(lib, block(width, 2, bpp, bpp * width - 1)) == ROW_STRIDE
        assert agree(lib, block(width, 2, bpp, bpp * width)) == OK


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_span_edge(lib, bpp):
    for width in (1, 640, ANY):
        exact = MAX_SPAN - bpp * width                # height 2: the span is row_stride + bpp * width
        assert span_of(block(width, 2, bpp, exact)) == MAX_SPAN
        assert agree(lib, block(width, 2, bpp, exact)) == OK
        assert agree(lib, block(width, 2, bpp, exact + 1)) == SPAN
        if width < ANY:                               # (32767 rows of 32767 colour pixels span more at any stride)
            last = (MAX_SPAN - bpp * width) // (ANY - 1)   # height 32767: the largest stride within the limit
            assert last >= bpp * width
            assert agree(lib, block(width, ANY, bpp, last)) == OK
            assert agree(lib, block(width, ANY, bpp, last + 1)) == SPAN
        for row_stride in (bpp * width, bpp * width + 65536, MAX_SPAN):   # one row: a stride that holds it is as good as any
            assert agree(lib, block(width, 1, bpp, row_stride)) == OK


@pytest.mark.parametrize("max_w,max_h", [CONTEXT, (ANY, ANY)])
def test_side_limits(lib, max_w, max_h):
    for width in (0, 1, max_w, max_w + 1):
        want = OK if 1 <= width <= max_w else SIDE
        assert agree(lib, block(width, 1, 3, 3 * ANY + 3), max_w, max_h) == want
    for height in (0, 1, max_h, max_h + 1):
        want = OK if 1 <= height <= max_h else SIDE
        assert agree(lib, block(1, height, 3, 3), max_w, max_h) == want
    assert agree(lib, block(-1, -1, 1, 1), max_w, max_h) == SIDE


def test_frame_count(lib):
    for n in (0, -1):
        assert agree(lib, block(4, 4, 1, 4, 16, n)) == COUNT
    assert agree(lib, block(4, 4, 1, 4, 16, 1)) == OK


def test_extent(lib):
    for frame_stride in (0, 1 << 40):     # a single frame: its stride is ignored
        b = block(5, 3, 3, 20, frame_stride, 1)
        assert lib.frames_emul_extent(C.byref(b)) == extent_of(b) == 2 * 20 + 15
    b = block(5, 3, 3, 20, 1000, 3)
    assert lib.frames_emul_extent(C.byref(b)) == extent_of(b) == 2 * 1000 + 2 * 20 + 15   # the last byte is BASE + 2054
    big = block(ANY, ANY, 4, 4 * ANY, 1 << 40, 3)
    assert lib.frames_emul_extent(C.byref(big)) == extent_of(big)


def both_ways(lib, a, b):
    got = lib.frames_emul_intersect(C.byref(a), C.byref(b))
    assert got == lib.frames_emul_intersect(C.byref(b), C.byref(a)) == int(intersect_of(a, b)) == int(intersect_of(b, a))
    return bool(got)


def test_intersection(lib):
    src = block(640, 480, 3, 1920, 1920 * 480, 2)
    end = BASE + extent_of(src)
    # the same shape; levels' GRAY plane; orient's turned frame; a padded one
    shapes = [(640, 480, 3, 1920, 1920 * 480), (640, 480, 1, 640, 640 * 480), (480, 640, 3, 1440, 1440 * 640), (640, 480, 3, 2048, 1 << 20)]
    for width, height, bpp, row_stride, frame_stride in shapes:
        dst = block(width, height, bpp, row_stride, frame_stride, 2, p=end)
        assert not both_ways(lib, src, dst)            # behind the source: touching
        dst.p = end - 1
        assert both_ways(lib, src, dst)                # its first byte is the source's last
        dst.p = BASE - extent_of(dst)
        assert not both_ways(lib, src, dst)            # in front of it: touching
        dst.p += 1
        assert both_ways(lib, src, dst)
    assert both_ways(lib, src, block(16, 16, 3, 1920, 0, 1, p=BASE + 10 * 1920 + 30))   # strictly inside
    assert both_ways(lib, src, block(640, 480, 3, 1920, 1920 * 480, 2))                  # identical
    assert both_ways(lib, src, block(1, 1, 1, 1, 0, 1, p=BASE + 1920 - 1))               # in a gap between rows: the block's too


def test_dwords(lib):
    p, row_stride, frame_stride = BASE, 1920, 1920 * 480
    assert lib.frames_emul_dwords(p, row_stride, frame_stride) == 1
    assert lib.frames_emul_dwords(p, row_stride, 0) == 1
    for odd in (1, 2, 3):
        for dp, dr, df in set(itertools.permutations((odd, 0, 0))):
            assert lib.frames_emul_dwords(p + dp, row_stride + dr, frame_stride + df) == 0, (dp, dr, df)

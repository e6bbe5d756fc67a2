"""CPU test of hd.h::grey_sum16, the 16-bit sum whose byte 1 is the grey value the frame binarise kernel stores: for all 2^24
(B, G, R) triples and both byte orders of the source pixel it must give BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14, and
the sum and its low part must fit 16 bits -- the kernel keeps two sums in one register and picks the grey bytes with one permute.
tests/emul/grey_pack_emul.cpp builds the function for the host."""
import ctypes as C

import pytest

from hostbuild import host_core


def build_lib():
    l = host_core("grey_pack_emul")
    l.gp_sweep.restype = C.c_longlong
    l.gp_sweep.argtypes = [C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    return l


@pytest.fixture(scope="module")
def lib():
    return build_lib()


@pytest.mark.parametrize("rev", [0, 1], ids=["bgr", "rgb"])
def test_byte_1_of_the_sum_is_bgr2gray_for_every_pixel(lib, rev):
    max_t, max_l = C.c_uint(0), C.c_uint(0)
    assert lib.gp_sweep(rev, C.byref(max_t), C.byref(max_l)) == 0
    # the bounds the packing rests on, and that the sweep met the pixel that reaches them (white)
    assert max_t.value < 65536 and max_l.value < 65536
    assert max_t.value == 255 * 255 + 128 + 255 and max_l.value == 256 * 255

"""CPU tests of the bit neighbour plane (hd.h: 16x14-pixel tiles with a one-pixel apron) the binarise kernels write and the
border followers read.  tests/emul/bitplane_emul.cpp is built twice -- with the product's bit plane and with the host
emulation's raster byte plane -- and both builds read the same random binary images: every pixel's mask through the
readers, and every plausible border start through the run test, the look behind and the walks of trace_core.h."""
import ctypes as C

import numpy as np
import pytest

from helpers import P
from hostbuild import host_core


def _lib(tiled):
    lib = host_core("bitplane_emul", tiled=tiled)
    lib.bp_plane_bytes.restype = C.c_longlong
    lib.bp_check_readers.restype = C.c_longlong
    return lib


@pytest.fixture(scope="module")
def libs():
    return _lib(True), _lib(False)


def _plane(lib, b):
    sh, sw = b.shape
    plane = np.zeros(int(lib.bp_plane_bytes(sw, sh)) + 16, np.uint8)   # (+16: a 12-byte window read at the last row stays inside)
    lib.bp_make_plane(P(b), sw, sh, P(plane))
    return plane


def _readers(lib, b, plane):
    sh, sw = b.shape
    masks = np.zeros((sh, sw), np.uint8)
    bad = lib.bp_check_readers(P(b), sw, sh, P(plane), P(masks))
    return bad, masks


def _walks(lib, b, plane):
    sh, sw = b.shape
    cap = b.size + 16
    out = np.zeros((cap, 16), np.int32)
    n = lib.bp_walks(P(b), sw, sh, P(plane), P(out), cap)
    assert n >= 0
    return out[:n]


def _images(rng):
    """random binary images of odd and even sizes; 1-pixel-wide lines and single pixels at tile and plane edges"""
    for trial in range(120):
        h, w = int(rng.integers(3, 75)), int(rng.integers(3, 75))
        dens = rng.choice([0.05, 0.3, 0.5, 0.7, 0.95])
        b = (rng.random((h, w)) < dens).astype(np.uint8)
        if trial % 4 == 1:   # blocky: long straight borders
            k = int(rng.integers(2, 6))
            b = np.kron((rng.random((h // k + 1, w // k + 1)) < dens).astype(np.uint8), np.ones((k, k), np.uint8))[:h, :w]
        if trial % 4 == 2:   # sparse 1-px features on tile rows / columns and next to the plane's edges
            b = np.zeros((h, w), np.uint8)
            for x in [c for c in (1, 2, 14, 15, 16, 17, 30, 31, 32, 33, w - 3, w - 2) if 0 < c < w - 1]:
                b[1:h - 1, x] = rng.random(h - 2) < 0.8
            for y in [r for r in (1, 2, 12, 13, 14, 15, 27, 28, 29, h - 3, h - 2) if 0 < r < h - 1]:
                b[y, 1:w - 1] |= (rng.random(w - 2) < 0.8).astype(np.uint8)
        if trial % 4 == 3:   # checkerboard noise: every neighbour bit pattern
            b = ((np.add.outer(np.arange(h), np.arange(w)) & 1) ^ (rng.random((h, w)) < 0.15)).astype(np.uint8)
        yield np.ascontiguousarray(b * 255)
    yield np.ascontiguousarray(((np.random.default_rng(7).random((270, 481)) < 0.55) * 255).astype(np.uint8))
    yield np.full((30, 48), 255, np.uint8)


def test_plane_size_is_a_bit_per_pixel_plus_the_apron(libs):
    tiled, raster = libs
    assert tiled.bp_plane_bytes(1920, 1080) == 120 * 78 * 64   # 0.6 MB against 2.07 MB of mask bytes
    assert tiled.bp_plane_bytes(17, 14) == 2 * 64 and tiled.bp_plane_bytes(16, 15) == 2 * 64
    assert raster.bp_plane_bytes(20, 10) == 200


def test_mask_of_every_pixel_equals_the_byte_plane(libs):
    tiled, raster = libs
    for b in _images(np.random.default_rng(3)):
        pt, pr = _plane(tiled, b), _plane(raster, b)
        bad_t, mt = _readers(tiled, b, pt)
        bad_r, mr = _readers(raster, b, pr)
        assert bad_t == 0 and bad_r == 0, b.shape
        assert (mt == mr).all(), b.shape


def test_followers_see_the_same_borders_on_both_planes(libs):
    tiled, raster = libs
    starts = 0
    for b in _images(np.random.default_rng(5)):
        wt, wr = _walks(tiled, b, _plane(tiled, b)), _walks(raster, b, _plane(raster, b))
        assert wt.shape == wr.shape, b.shape
        # column 0 is the scan position, which depends on the plane's row stride; the rest must match exactly
        assert (wt[:, 1:] == wr[:, 1:]).all(), (b.shape, np.argwhere(wt[:, 1:] != wr[:, 1:])[:4])
        assert (wt[:, 3] == wt[:, 2]).all()      # the bit scan of the run test decides as the byte test does
        assert (wt[:, 15] == 1).all()            # run skipping changes nothing
        starts += len(wt)
    assert starts > 10000

"""The levels core (opencv-ar_amd/csrc/levels_core.h) in its host build (tests/emul/levels_emul.cpp), without a GPU: the step against a
numpy restatement byte for byte, the pieces of the definition one by one, the plan the kernels share with it, the exposure chain through
the oracle, the stand-alone program under the sanitizers, and the ABI.  tests/test_gpu_levels.py holds the kernels to this build byte
for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import levels_chain as LC
from hostbuild import run_sanitized


@pytest.fixture(scope="module")
def L():
    return LC.build_emul()


def test_constants_agree_with_the_core(L):
    assert (L.levels_slab_rows_emul(), L.levels_seg_w_emul(), L.levels_seg_h_emul(), L.levels_ws_frames_emul()) == (LC.SLAB_ROWS, LC.SEG_W, LC.SEG_H, LC.WS_FRAMES)
    assert L.levels_ws_bytes_emul() == LC.WS_BYTES == 20 * 2 ** 20
    p = LC.Params()
    L.levels_default_params_emul(C.addressof(p))
    assert LC.as_tuple(p) == LC.as_tuple(LC.params()) == (1, 1, 10000, 10000, 2048)


# ---- the step against numpy ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
def test_frames_against_numpy(L, fmt):
    """guarded frames with padded rows, aligned and odd layouts, every shared shape and grid under every setting of the knobs: numpy's
    plane of the frame's grey, every guard byte kept, the source untouched"""
    for k, (w, h, tiles) in enumerate(LC.SHAPES):
        for q, (lo, hi, gain) in enumerate(LC.KNOBS):
            aligned = (k + q) % 2 == 0
            p = LC.params(tiles, lo, hi, gain)
            src = FK.pix_layout(2, w, h, fmt, aligned, seed=k + 1)
            dst = LC.dst_layout(src, aligned)
            before = src.buf.copy()
            rc, got = LC.host_levels(L, src, dst, p)
            assert rc == 0 and (src.buf == before).all()
            assert (got[~dst.pixel_mask()] == FK.GUARD).all()
            for f in range(src.n):
                want = LC.np_levels_params(LC.np_grey(src.view(f), fmt), p)
                bad = np.argwhere(dst.view(f, got)[..., 0] != want)
                assert bad.size == 0, (fmt, w, h, tiles, LC.KNOBS[q], bad[:4].tolist())


@pytest.mark.parametrize("name", ["zeros", "mid", "ones", "two", "ramp", "halves"])
def test_special_frames_against_numpy(L, name):
    """constant frames of 0, 128 and 255 (both clamps of the gain cap), a two-valued frame, a frame over 0 .. 255, a frame whose lo
    exceeds its hi before the cap: numpy's bytes under every setting of the knobs, with one tile and with a grid"""
    for w, h, tiles in [(37, 23, (1, 1)), (37, 23, (4, 3)), (16, 16, (8, 8))]:
        g = LC.special_frames(w, h)[name]
        for lo, hi, gain in LC.KNOBS:
            p = LC.params(tiles, lo, hi, gain)
            got, want = LC.host_levels_image(L, g, p), LC.np_levels_params(g, p)
            assert (got == want).all(), (name, w, h, tiles, lo, hi, gain, np.argwhere(got != want)[:4].tolist())


def test_bounds_and_the_gain_cap(L):
    """lo and hi before and after the cap on histograms written by hand"""
    out = np.zeros(4, np.int32)

    def bounds(values, lo=10000, hi=10000, gain=2048):
        hist = np.bincount(np.asarray(values), minlength=256).astype(np.uint32)
        p = LC.params((1, 1), lo, hi, gain)
        L.levels_bounds_emul(hist.ctypes.data, C.addressof(p), out.ctypes.data)
        want = LC.np_bounds(values, lo, hi)
        assert tuple(out[:2]) == want and tuple(out[2:]) == LC.np_cap(*want, gain)
        return tuple(int(v) for v in out)

    assert bounds([0] * 10) == (0, 0, 0, 32)                 # minr = 32 at a gain of 8; (0 + 0 - 32) >> 1 = -16 -> 0
    assert bounds([255] * 10) == (255, 255, 223, 255)        # (510 - 32) >> 1 = 239 -> 255 - 32
    assert bounds([128] * 10) == (128, 128, 112, 144)
    assert bounds([128] * 10, gain=256) == (128, 128, 0, 255)
    assert bounds([128] * 10, gain=65280) == (128, 128, 127, 128)      # minr = 1: (256 - 1) >> 1
    assert bounds([10, 240], 500000, 500000) == (240, 10, 109, 141)    # lo > hi before the cap
    assert bounds([10, 240], 0, 0) == (10, 240, 10, 240)
    assert bounds(list(range(200)), 10000, 10000) == (2, 197, 2, 197)  # k = 2: two values clipped at each end
    assert bounds(list(range(100)) * 3, 0, 500000) == (0, 49, 0, 49)   # k_hi = 150 = #{g >= 50}: not above it
    assert bounds([7, 9], 0, 0, gain=65280) == (7, 9, 7, 9) and bounds([7, 8], 0, 0, gain=65279) == (7, 8, 6, 8)   # minr 1 and 2


def test_lut_is_the_rounded_stretch(L):
    rng = np.random.default_rng(3)
    lut = np.zeros(256, np.uint8)
    for _ in range(50):
        vals = rng.integers(rng.integers(0, 100), rng.integers(101, 256), 500)
        p = LC.params((1, 1), int(rng.integers(0, 500001)), int(rng.integers(0, 500001)), int(rng.integers(256, 65281)))
        hist = np.bincount(vals, minlength=256).astype(np.uint32)
        L.levels_lut_emul(hist.ctypes.data, C.addressof(p), lut.ctypes.data)
        assert (lut == LC.np_lut(vals, p.low_ppm, p.high_ppm, p.max_gain_q8)).all()
        lo, hi = LC.np_cap(*LC.np_bounds(vals, p.low_ppm, p.high_ppm), p.max_gain_q8)
        assert lut[lo] == 0 and lut[hi] == 255 and (np.diff(lut.astype(int)) >= 0).all() and (lut[:lo] == 0).all() and (lut[hi:] == 255).all()
        v = np.arange(lo, hi + 1)
        assert np.abs(lut[lo:hi + 1] - (v - lo) * 255.0 / (hi - lo)).max() <= 0.5


def test_axis_against_numpy(L):
    """the two tiles and the weight of every pixel of an axis: numpy's, 0 at the first tile's centre and towards the border, 256 from
    the last tile's centre on, never descending inside a cell"""
    out = np.zeros(3, np.int32)
    for extent, tiles in [(1, 1), (2, 2), (7, 7), (16, 8), (37, 4), (37, 5), (23, 3), (23, 2), (41, 8), (67, 8), (300, 16), (1920, 8), (32767, 16)]:
        i0, i1, w = LC.np_axis(extent, tiles)
        xs = range(extent) if extent < 5000 else list(range(0, extent, 97)) + [extent - 1]
        for x in xs:
            L.levels_axis_emul(x, extent, tiles, out.ctypes.data)
            assert tuple(out) == (i0[x], i1[x], w[x]), (extent, tiles, x)
        assert w[0] == 0 or tiles > extent // 2 + 1
        if tiles > 1:
            assert i1[-1] == tiles - 1 and w[-1] == 256 and (w[i0 == 0][:1] == 0).all()


# ---- further properties ----------------------------------------------------------------------------------------------------------------

def test_one_tile_is_the_lut_of_the_grey(L):
    rng = np.random.default_rng(5)
    g = rng.integers(30, 180, (23, 37), dtype=np.uint8)
    src = FK.pix_layout(1, 37, 23, "gray", True)
    src.view(0)[..., 0] = g
    rc, got, luts = LC.host_levels(L, src, LC.dst_layout(src, True), LC.params(), want_luts=True)
    assert rc == 0 and (LC.dst_layout(src, True).view(0, got)[..., 0] == luts[0, 0][g]).all()
    assert (luts[0, 0] == LC.np_lut(g, 10000, 10000, 2048)).all()


@pytest.mark.parametrize("fmt", ["bgr", "rgb", "bgra", "rgba"])
def test_colour_formats_give_the_result_of_their_grey_plane(L, fmt):
    rng = np.random.default_rng(6)
    px = rng.integers(0, 256, (23, 37, FK.BPP[FK.FORMATS[fmt]]), dtype=np.uint8)
    grey = LC.np_grey(px, fmt)
    for a, b, c in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (17, 200, 90)]:
        order = (a, b, c) if fmt in ("bgr", "bgra") else (c, b, a)
        assert L.levels_grey_emul(*order, FK.FORMATS[fmt]) == (1868 * a + 9617 * b + 4899 * c + 8192) >> 14
    for p in (LC.params(), LC.params((4, 3)), LC.params((5, 2), 0, 50000, 1024)):
        assert (LC.host_levels_image(L, px, p, fmt=fmt) == LC.host_levels_image(L, grey, p)).all()


def test_no_clipping_on_a_full_range_frame_is_the_identity(L):
    rng = np.random.default_rng(7)
    g = rng.integers(0, 256, (23, 37), dtype=np.uint8)
    g[0, 0], g[-1, -1] = 0, 255
    for gain in (256, 2048, 65280):
        assert (LC.host_levels_image(L, g, LC.params((1, 1), 0, 0, gain)) == g).all()
    # and with ppm = 0 and no cap reached it is the min-max stretch, rounded to nearest
    g2 = (g.astype(int) * 100 // 255 + 60).astype(np.uint8)
    want = np.floor((g2.astype(np.float64) - g2.min()) * 255 / (int(g2.max()) - int(g2.min())) + 0.5)
    assert (LC.host_levels_image(L, g2, LC.params((1, 1), 0, 0, 2048)) == want).all()


def test_refusals_of_the_host_call(L):
    px, out = np.zeros(64, np.uint8), np.full(64, FK.GUARD, np.uint8)

    def call(w=4, h=4, srs=12, fmt=0, drs=4, n=1, p=None):
        return L.levels_emul(px.ctypes.data, w, h, srs, srs * max(h, 1), fmt, out.ctypes.data, drs, drs * max(h, 1), n, None if p is None else C.addressof(p),
                             None, None)

    bad = [dict(w=0), dict(h=0), dict(w=32768, srs=3 * 32768), dict(h=32768), dict(srs=11), dict(drs=3), dict(fmt=5), dict(fmt=-1), dict(n=0), dict(n=-1)]
    bad += [dict(p=LC.params(t)) for t in [(0, 1), (1, 0), (17, 1), (1, 17), (16, 5), (5, 1), (1, 5)]]
    bad += [dict(p=LC.params((1, 1), *k)) for k in [(-1, 0, 2048), (0, -1, 2048), (500001, 0, 2048), (0, 500001, 2048), (0, 0, 255), (0, 0, 65281)]]
    for kw in bad:
        assert call(**kw) == FK.E_ARG, kw
    assert (out == FK.GUARD).all()
    assert call() == 0 and call(p=LC.params((4, 4), 0, 500000, 65280)) == 0


# ---- the plan the kernels share --------------------------------------------------------------------------------------------------------

def test_segments_cover_every_axis_once_inside_one_cell(L):
    """the apply kernel's segments: every pixel once and in order, each segment inside one cell of the tile-centre lattice, the
    kernel's weight that of the definition (levels_segments_emul checks every pixel), the count what the cells' lengths give"""
    for extent, tiles in [(1, 1), (2, 2), (7, 7), (16, 8), (37, 4), (37, 5), (67, 8), (300, 1), (300, 16), (1920, 1), (1920, 4), (1920, 8), (1080, 8), (32767, 1), (32767, 16)]:
        for seg in (LC.SEG_W, LC.SEG_H):
            out = np.zeros(3 * (extent // seg + 17), np.int32)
            n = L.levels_segments_emul(extent, tiles, seg, out.ctypes.data)
            assert n >= 1, (extent, tiles, seg)
            segs = out[:3 * n].reshape(n, 3)
            i0, _, _ = LC.np_axis(extent, tiles)
            assert sorted(set(segs[:, 0].tolist())) == sorted(set(i0.tolist())) == list(range(max(tiles - 1, 1)))
            assert n == sum(-(-int((i0 == k).sum()) // seg) for k in range(max(tiles - 1, 1)))


def test_the_slabs_of_the_tall_case():
    """64 x 300 with one tile, the GPU test's case: the plan cuts the tile into ceil(300 / SLAB_ROWS) row slabs, at least three, the
    last one partial"""
    assert -(-300 // LC.SLAB_ROWS) >= 3 and 300 % LC.SLAB_ROWS != 0


# ---- the chain, on the oracle only -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(L):
    """exposure -> records recovered (raw, global, 4x4, 8x8) out of the oracle's records on the undimmed scenes, the planes by the
    host core"""
    tpls = H.oracle_templates()
    scenes = LC.chain_scenes()
    truth = {name: H.oracle_registration(bgr, tpls, H.oracle_camera(bgr.shape[1], bgr.shape[0]))[0] for name, bgr in scenes}
    totals = {}
    for e in LC.EXPOSURES:
        tot = [0, 0, 0, 0]
        for name, bgr in scenes:
            x = LC.expose(bgr, e)
            planes = [LC.np_grey(x, "bgr"), LC.host_levels_image(L, x), LC.host_levels_image(L, x, LC.params((4, 4))), LC.host_levels_image(L, x, LC.params((8, 8)))]
            for k, plane in enumerate(planes):
                tot[k] += LC.recovered(LC.oracle_on_grey(plane, tpls), truth[name])
        totals[e] = tuple(tot)
        print("%-8s raw %2d  global %2d  4x4 %2d  8x8 %2d  of %d (measured %s)" % ((e,) + totals[e] + (LC.CHAIN_RECORDS, LC.CHAIN_MEASURED[e])))
    return dict(records=sum(len(v) for v in truth.values()), totals=totals)


def test_the_exposure_chain_on_the_cpu(chain):
    """the library's synthetic scenes under six wrong exposures: what the oracle recovers (same template, corners within 2 px) on the
    raw frames, after global levels, and after levels per tile.  A uniformly wrong exposure comes back with one map per frame; an
    exposure that changes across the image needs the tiles, which is what the split exposure shows.  Measured (LC.CHAIN_MEASURED, of
    14): dark 0 / 11 / 11 / 10, bright 0 / 13 / 12 / 10, flat 0 / 11 / 11 / 10, halfdark 8 / 7 / 12 / 10, ramp 5 / 9 / 12 / 10,
    split 0 / 0 / 10 / 9 for raw / global / 4x4 / 8x8."""
    t = chain["totals"]
    assert chain["records"] == LC.CHAIN_RECORDS
    for e in LC.RAW_ZERO:
        assert t[e][0] == 0, (e, t[e])
    for e, bar in LC.GLOBAL_BAR.items():
        assert t[e][1] >= bar, (e, t[e])
    for e, bar in LC.TILED_BAR.items():
        assert t[e][2] >= bar, (e, t[e])
    assert t["split"][1] <= LC.GLOBAL_SPLIT_AT_MOST, t["split"]


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers():
    """tests/emul/levels_emul.cpp with its own main, built with -fsanitize=address,undefined and run as a program: sides 1 .. 32767,
    every pixel size, grids up to 16 tiles an axis, the extremes of the knobs, random, constant and two-valued frames on heap blocks of
    exactly the bytes a call may touch"""
    run_sanitized("levels_emul", "LEVELS_EMUL_MAIN", ", 0 bad", timeout=600)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------

def test_abi_and_python_names():
    """the two entry points are declared in the header and exported by the library; the module's struct, defaults and checks agree with
    the header"""
    import __graft_entry__ as g
    g.build()
    import opencv_ar_amd as oa
    header = open(os.path.join(H.ROOT, "include", "ocvar_hip.h")).read()
    lib = oa.hip_lib()
    for name in ("ocvar_hip_levels", "ocvar_hip_levels_default_params"):
        assert re.search(r"\bint %s\(" % name, header) and name in oa.HIP_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int tiles_x, tiles_y, low_ppm, high_ppm, max_gain_q8;", header)
    assert [f[0] for f in oa.LevelsParams._fields_] == [f[0] for f in LC.Params._fields_] and C.sizeof(oa.LevelsParams) == 20
    p = oa.LevelsParams(9, 9, 9, 9, 9)
    assert lib.ocvar_hip_levels_default_params(C.byref(p)) == 0 and lib.ocvar_hip_levels_default_params(None) == FK.E_ARG
    assert LC.as_tuple(p) == LC.as_tuple(oa.levels_params()) == (1, 1, 10000, 10000, 2048)
    assert LC.as_tuple(oa.levels_params((4, 3), 0, 500000, 1.0)) == (4, 3, 0, 500000, 256) and oa.levels_params(max_gain=255).max_gain_q8 == 65280
    assert hasattr(oa.Detector, "levels")
    for kw in (dict(tiles=(0, 1)), dict(tiles=(17, 1)), dict(tiles=(16, 5)), dict(tiles=3), dict(low_ppm=-1), dict(high_ppm=500001), dict(low_ppm=0.5),
               dict(max_gain=0.5), dict(max_gain=256), dict(max_gain=True)):
        with pytest.raises(ValueError):
            oa.levels_params(**kw)

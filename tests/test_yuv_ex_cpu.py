"""The extended YUV conversion core (opencv-ar_amd/csrc/yuv_ex_core.h) on the host (tests/yuv_ex_chain.py builds it): the tables
against their float64 formula, the formulas against a numpy restatement and against the float64 matrices, the two frame loops on
every layout, depth, format and border case with guard bytes around every row, plane and frame, what the new ground promises
(the old calls' bytes where both apply, NV21, I444, the low bits of P010, P016 against 8 bits, the round trip), the refusals of
the host call, the chain through the oracle, the sanitizer program and the ABI surface.  tests/test_gpu_yuv_ex.py holds the
kernels to this build byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bayer_chain as BC
import frame_kit as FK
import helpers as H
import levels_chain as LC
import overlay_chain as OC
import yuv_chain as YC
import yuv_ex_chain as YX
from hostbuild import run_sanitized

MATS, RNGS = list(YX.MATRICES), list(YX.RANGES)
TABLES = [(m, r, b) for b in YX.DEPTHS for m in MATS for r in RNGS]
NEW8 = [("bt601", "full", 8), ("bt709", "full", 8), ("bt2020", "full", 8), ("bt2020", "limited", 8)]   # the 8-bit tables new to the _ex calls
N24 = 1 << 24


def tid(t):
    return "%s-%s-%d" % t


@pytest.fixture(scope="module")
def L():
    return YX.build_emul()


@pytest.fixture(scope="module")
def LY():
    return YC.build_emul()


def host_bgr(L, t, yuv):
    """[n, 3] samples Y U V -> [n, 3] B G R of the host core, int64"""
    yuv = np.ascontiguousarray(yuv, np.uint16)
    out = np.zeros((len(yuv), 3), np.uint8)
    L.yuv_ex_to_bgr_emul(YX.MATRICES[t[0]], YX.RANGES[t[1]], t[2], yuv.ctypes.data, len(yuv), out.ctypes.data)
    return out.astype(np.int64)


def host_yuv(L, t, bgr, log2n):
    """[n, 3] colours B G R as constant blocks of 2^log2n pixels -> [n, 3] Y U V of the host core, int64"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    out = np.zeros((len(bgr), 3), np.uint16)
    assert L.yuv_ex_from_bgr_emul(YX.MATRICES[t[0]], YX.RANGES[t[1]], t[2], log2n, bgr.ctypes.data, len(bgr), out.ctypes.data) == 0
    return out.astype(np.int64)


def all_triples(dtype):
    """[2^24, 3]: the three bytes of every index, most significant first"""
    i = np.arange(N24, dtype=np.int32)
    out = np.empty((N24, 3), dtype)
    out[:, 0], out[:, 1], out[:, 2] = i >> 16, (i >> 8) & 255, i & 255
    return out


def half_up(x, top):
    return np.clip(np.floor(x + 0.5), 0, top).astype(np.int64)


# ---- 1. the tables ------------------------------------------------------------------------------------------------------------------------

def test_the_tables_are_the_float64_formula_rounded(L):
    for m, r, b in TABLES:
        got, want = YX.host_table(L, m, r, b), YX.table(m, r, b)
        assert got == want, (m, r, b)
        assert max(abs(got[k]) for k in YC.COEF_NAMES) < 1 << 23, (m, r, b)   # (the 24-bit multiplier of the kernels is exact)
        assert got["y_off"] == (0 if r == "full" else 16 << (b - 8)) and got["c_mid"] == 128 << (b - 8)
        assert got["out_shift"] == 28 - b and got["word_shift"] == 16 - b and got["out_y_off"] == (0 if r == "full" else 16 << 20)
    for m in ("bt601", "bt709"):   # the existing tables, verbatim
        got = YX.host_table(L, m, "limited", 8)
        assert {k: got[k] for k in YC.COEF_NAMES} == YC.COEF[m]
    # the stated formula, written out once more for one table: BT.2020 full range at 10 bits
    kr, kb = 0.2627, 0.0593
    kg, s = 1 - kr - kb, 255.0 / 1023.0
    got = YX.host_table(L, "bt2020", "full", 10)
    assert got["cy"] == round(s * 2 ** 20) and got["cvr"] == round(2 * (1 - kr) * s * 2 ** 20) and got["cub"] == round(2 * (1 - kb) * s * 2 ** 20)
    assert got["cug"] == round(-2 * kb * (1 - kb) / kg * s * 2 ** 20) and got["gy"] == round(kg / (s * 4) * 2 ** 20)


# ---- 2. the formulae against float64 --------------------------------------------------------------------------------------------------------

def to_colour_check(L, t, yuv):
    """the host core on [n, 3] samples: the numpy restatement exactly, the float64 matrix within 1 level -> the share that differs"""
    tab, f = YX.table(*t), YX.float_model(*t)
    got = host_bgr(L, t, yuv)
    Y, U, V = (yuv[:, c].astype(np.int64) for c in range(3))
    B, G, R = YX.np_to_bgr(tab, Y, U, V)
    assert (got[:, 0] == B).all() and (got[:, 1] == G).all() and (got[:, 2] == R).all(), t
    y, u, v = np.maximum(Y - f["y_off"], 0) * f["cy"], U - f["c_mid"], V - f["c_mid"]
    differ = np.zeros(len(yuv), bool)
    for c, want in ((2, y + f["cvr"] * v), (1, y + f["cvg"] * v + f["cug"] * u), (0, y + f["cub"] * u)):
        d = np.abs(got[:, c] - half_up(want, 255))
        assert d.max() <= 1, (t, "BGR"[c], int(d.max()))
        differ |= d > 0
    return differ.mean()


def to_yuv_check(L, t, bgr):
    """the same for colour to YUV, for blocks of 1, 2 and 4 equal pixels"""
    tab, f = YX.table(*t), YX.float_model(*t)
    top = (1 << t[2]) - 1
    B, G, R = (bgr[:, c].astype(np.int64) for c in range(3))
    got = host_yuv(L, t, bgr, 2)
    for log2n in (0, 1):
        assert (host_yuv(L, t, bgr, log2n) == got).all()   # (a constant block's samples do not depend on its size)
    assert (got[:, 0] == YX.np_luma(tab, B, G, R)).all()
    U, V = YX.np_chroma(tab, B << 2, G << 2, R << 2, 2)
    assert (got[:, 1] == U).all() and (got[:, 2] == V).all()
    differ = np.zeros(len(bgr), bool)
    for c, want in ((0, f["ry"] * R + f["gy"] * G + f["by"] * B + f["y_off"]), (1, f["ru"] * R + f["gu"] * G + f["bu"] * B + f["c_mid"]),
                    (2, f["rv"] * R + f["gv"] * G + f["bv"] * B + f["c_mid"])):
        d = np.abs(got[:, c] - half_up(want, top))
        assert d.max() <= 1, (t, "YUV"[c], int(d.max()))
        differ |= d > 0
    # what the range promises: greys have no colour; limited Y spans 16 .. 235 and chroma 16 .. 240 (times 2^(n-8)), full 0 .. 2^n - 1
    grey = got[(B == G) & (G == R)]
    assert (grey[:, 1:] == f["c_mid"]).all()
    return differ.mean(), got


@pytest.mark.parametrize("t", NEW8, ids=tid)
def test_8_bit_formulae_on_every_input(L, t):
    """All 2^24 (Y, U, V) and all 2^24 colours for each 8-bit table the _ex calls add: the numpy restatement exactly, and every
    result within 1 level of the rounded float64 value.  Measured share of inputs with a result that differs from the float64
    one, to colour / to YUV: BT.601 full 0.053 % / 0.060 %, BT.709 full 0.000 % / 0.012 %, BT.2020 full 0.006 % / 0.026 %, BT.2020
    limited 0.007 % / 0.017 %."""
    a = to_colour_check(L, t, all_triples(np.uint16))
    b, got = to_yuv_check(L, t, all_triples(np.uint8))
    print("%s: %.4f %% of all (Y, U, V) and %.4f %% of all colours differ from the rounded float64 value" % (tid(t), 100 * a, 100 * b))
    up = 1 << (t[2] - 8)
    if t[1] == "full":
        assert got[:, 0].min() == 0 and got[:, 0].max() == 255 and got[:, 1:].min() <= 1 and got[:, 1:].max() == 255
    else:
        assert got[:, 0].min() == 16 * up and got[:, 0].max() == 235 * up and got[:, 1:].min() == 16 * up and got[:, 1:].max() == 240 * up


def edge_values(top, extra=()):
    mid = (top + 1) // 2
    return sorted({0, 1, mid - 1, mid, mid + 1, top - 1, top, *extra})


@pytest.mark.parametrize("m", MATS)
@pytest.mark.parametrize("r", RNGS)
def test_10_bit_formulae_on_a_grid(L, m, r):
    """Every Y against (U, V) on a grid that holds 0, 1, 511, 512, 513, 1022, 1023 and 33 evenly spread values; the colours: every
    channel on the byte's edges and 52 evenly spread values.  Measured share that differs from the float64 value: to colour 0.015 % ..
    0.043 %, to YUV 0.005 % .. 0.090 %, over the six tables."""
    t = (m, r, 10)
    grid = np.array(sorted(set(edge_values(1023)) | set(np.linspace(0, 1023, 33).round().astype(int).tolist())))
    assert len(grid) >= 25 + 7 and {0, 1, 511, 512, 513, 1022, 1023} <= set(grid.tolist())
    Y, U, V = np.meshgrid(np.arange(1024), grid, grid, indexing="ij")
    a = to_colour_check(L, t, np.stack([Y.ravel(), U.ravel(), V.ravel()], 1).astype(np.uint16))
    ch = np.array(sorted(set(edge_values(255)) | set(range(0, 256, 5))))
    Bc, Gc, Rc = np.meshgrid(ch, ch, ch, indexing="ij")
    b, _ = to_yuv_check(L, t, np.stack([Bc.ravel(), Gc.ravel(), Rc.ravel()], 1).astype(np.uint8))
    print("%s: %.4f %% of the grid and %.4f %% of the colours differ from the rounded float64 value" % (tid(t), 100 * a, 100 * b))


@pytest.mark.parametrize("bits", [12, 16])
@pytest.mark.parametrize("m", MATS)
@pytest.mark.parametrize("r", RNGS)
def test_12_and_16_bit_formulae_on_edges_and_random_triples(L, m, r, bits):
    """The edges of every operand (0, 1, the centre and its neighbours, the top and its neighbour, the luma offset and its
    neighbours) in every combination, and 2^20 random triples (seed 12 / 16).  Measured share that differs from the float64 value,
    over the six tables of a depth: at 12 bits to colour 0.055 % .. 0.067 %, to YUV 0.064 % .. 0.43 %; at 16 bits to colour 0.75 % ..
    1.8 %, to YUV 0.57 % .. 4.2 % (a 16-bit level is 1 / 256 of an 8-bit one, and the coefficients' rounding is 0.09 of it)."""
    t = (m, r, bits)
    top = (1 << bits) - 1
    off = 16 << (bits - 8)
    e = np.array(edge_values(top, (off - 1, off, off + 1)))
    Y, U, V = np.meshgrid(e, e, e, indexing="ij")
    rng = np.random.default_rng(bits)
    yuv = np.concatenate([np.stack([Y.ravel(), U.ravel(), V.ravel()], 1), rng.integers(0, top + 1, (1 << 20, 3))]).astype(np.uint16)
    a = to_colour_check(L, t, yuv)
    e8 = np.array(edge_values(255))
    Bc, Gc, Rc = np.meshgrid(e8, e8, e8, indexing="ij")
    bgr = np.concatenate([np.stack([Bc.ravel(), Gc.ravel(), Rc.ravel()], 1), rng.integers(0, 256, (1 << 20, 3))]).astype(np.uint8)
    b, got = to_yuv_check(L, t, bgr)
    print("%s: %.4f %% of the triples and %.4f %% of the colours differ from the rounded float64 value" % (tid(t), 100 * a, 100 * b))
    assert got.max() == (top if r == "full" else 240 << (bits - 8))


@pytest.mark.parametrize("t", TABLES, ids=tid)
def test_chroma_of_mixed_blocks(L, t):
    """blocks of 1, 2 and 4 random pixels, of extreme ones and of one bright pixel among dark ones, from their channel sums"""
    tab = YX.table(*t)
    for log2n in (0, 1, 2):
        rng = np.random.default_rng(log2n)
        px = rng.integers(0, 256, (60000, 1 << log2n, 3))
        px[:20000] = rng.integers(0, 2, (20000, 1 << log2n, 3)) * 255
        px[20000:25000, 1:] = 0
        sums = np.ascontiguousarray(px.sum(1), np.int32)
        got = np.zeros((len(sums), 2), np.uint16)
        L.yuv_ex_chroma_emul(YX.MATRICES[t[0]], YX.RANGES[t[1]], t[2], log2n, sums.ctypes.data, len(sums), got.ctypes.data)
        U, V = YX.np_chroma(tab, sums[:, 0], sums[:, 1], sums[:, 2], log2n)
        assert (got[:, 0] == U).all() and (got[:, 1] == V).all(), (t, log2n)


# ---- 3. the frame loops ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("layout,bits", YX.LAYOUT_DEPTHS)
def test_yuv_to_frames_on_every_layout_depth_format_and_border(L, layout, bits, fmt):
    """aligned, and with an odd (16-bit samples: even) leading offset, row padding, a gap between the planes and between the frames;
    two frames; the six tables in turn"""
    for i, (W, Hh) in enumerate(YX.sizes_of(layout)):
        for aligned in (True, False):
            m, r = YX.variant(i + aligned)
            yuv = YX.YuvEx(2, W, Hh, layout, bits, aligned=aligned, seed=W + Hh, matrix=m, rng=r)
            dst = FK.pix_layout(2, W, Hh, fmt, aligned=aligned, fill=FK.GUARD)
            before = yuv.buf.copy()
            out = YX.host_to_frames(L, yuv, dst)
            assert (yuv.buf == before).all()
            assert (out[~dst.pixel_mask()] == FK.GUARD).all(), (W, Hh)
            for f in range(2):
                want = YX.np_frame_to_pixels(yuv.table(), fmt, *yuv.samples(f))
                assert (dst.view(f, out) == want).all(), (W, Hh, f, m, r, aligned)
                if dst.bpp == 4:
                    assert (dst.view(f, out)[..., 3] == 255).all()
            if fmt == "gray" and aligned:   # the library's grey of the BGR target, byte for byte
                bgr = FK.pix_layout(2, W, Hh, "bgr", aligned=True, fill=FK.GUARD)
                ob = YX.host_to_frames(L, yuv, bgr)
                for f in range(2):
                    b = bgr.view(f, ob).astype(np.int64)
                    assert (dst.view(f, out)[..., 0] == OC.grey_of(b[..., 0], b[..., 1], b[..., 2])).all()


@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("layout,bits", YX.LAYOUT_DEPTHS)
def test_frames_to_yuv_on_every_layout_depth_format_and_border(L, layout, bits, fmt):
    for i, (W, Hh) in enumerate(YX.sizes_of(layout)):
        for aligned in (True, False):
            m, r = YX.variant(i + 1 + aligned)
            src = FK.pix_layout(2, W, Hh, fmt, aligned=aligned, seed=W * Hh)
            yuv = YX.YuvEx(2, W, Hh, layout, bits, aligned=aligned, matrix=m, rng=r)
            before = src.buf.copy()
            out = YX.host_to_yuv(L, src, yuv)
            assert (src.buf == before).all()
            assert (out[~yuv.sample_mask()] == FK.GUARD).all(), (W, Hh)
            for f in range(2):
                want = YX.np_pixels_to_frame(yuv.table(), fmt, src.view(f), yuv.sub)
                for got_plane, want_plane in zip(yuv.samples(f, out), want):
                    assert (got_plane == want_plane).all(), (W, Hh, f, m, r, aligned)
                if bits > 8:   # the low bits of every word are written as zero
                    for k in range(2):
                        assert (yuv.words(f, k, out) & ((1 << (16 - bits)) - 1) == 0).all()
            if src.bpp == 4 and aligned:   # byte 3 of a source pixel is ignored
                other = src.buf.copy()
                for f in range(2):
                    src.view(f, other)[..., 3] ^= 0x5A
                assert (YX.host_to_yuv(L, src, yuv, buf=other) == out).all()


# ---- 4. equalities ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(YC.LAYOUTS))
@pytest.mark.parametrize("fmt", FK.FMTS)
def test_the_old_host_build_byte_for_byte_where_both_apply(L, LY, layout, fmt):
    """8 bits, limited range, BT.601 and BT.709, the four old layouts: whole buffers, both directions"""
    for i, (W, Hh) in enumerate(YC.SIZES):
        for m in ("bt601", "bt709"):
            aligned = bool((i + (m == "bt709")) % 2)
            old = YC.Yuv(2, W, Hh, layout, aligned=aligned, seed=W + Hh)
            new = YX.YuvEx(2, W, Hh, layout, 8, aligned=aligned, matrix=m)
            assert (old.lead, old.planes, old.frame_stride, old.y_pitch, old.c_pitch) == (new.lead, new.planes, new.frame_stride, new.y_pitch, new.c_pitch)
            dst = FK.pix_layout(2, W, Hh, fmt, aligned=aligned, fill=FK.GUARD)
            assert (YX.host_to_frames(L, new, dst, buf=old.buf) == YC.host_to_frames(LY, old, m, dst)).all(), (W, Hh, m)
            src = FK.pix_layout(2, W, Hh, fmt, aligned=aligned, seed=W)
            assert (YX.host_to_yuv(L, src, new) == YC.host_to_yuv(LY, src, m, YC.Yuv(2, W, Hh, layout, aligned=aligned))).all(), (W, Hh, m)


@pytest.mark.parametrize("fmt", ["bgr", "rgba", "gray"])
def test_nv21_is_nv12_with_the_chroma_bytes_exchanged(L, fmt):
    for i, (W, Hh) in enumerate(YX.SIZES):
        m, r = YX.variant(i)
        a, b = (YX.YuvEx(1, W, Hh, lay, 8, aligned=bool(i % 2), seed=W, matrix=m, rng=r) for lay in ("nv12", "nv21"))
        assert (a.buf == b.buf).all()
        c = b.plane_view(0, 1)
        c[:, 0::2], c[:, 1::2] = c[:, 1::2].copy(), c[:, 0::2].copy()
        dst = FK.pix_layout(1, W, Hh, fmt, aligned=True, fill=FK.GUARD)
        assert (YX.host_to_frames(L, a, dst) == YX.host_to_frames(L, b, dst)).all(), (W, Hh)
        src = FK.pix_layout(1, W, Hh, fmt, aligned=False, seed=W + 1)
        oa, ob = YX.host_to_yuv(L, src, a), YX.host_to_yuv(L, src, b)
        ca = a.plane_view(0, 1, oa)
        cb = b.plane_view(0, 1, ob)
        assert (a.plane_view(0, 0, oa) == b.plane_view(0, 0, ob)).all() and (ca[:, 0::2] == cb[:, 1::2]).all() and (ca[:, 1::2] == cb[:, 0::2]).all()
        assert fmt == "gray" or W < 8 or (ca[:, 0::2] != ca[:, 1::2]).any()   # (a grey source has no colour: U = V)


@pytest.mark.parametrize("fmt", ["bgr", "rgb", "gray"])
def test_i444_with_repeated_chroma_gives_i420s_colour(L, fmt):
    for i, (W, Hh) in enumerate(YX.SIZES):
        m, r = YX.variant(i)
        a = YX.YuvEx(1, W, Hh, "i420", 8, aligned=False, seed=W, matrix=m, rng=r)
        b = YX.YuvEx(1, W, Hh, "i444", 8, aligned=True, matrix=m, rng=r)
        Y, U, V = a.samples(0)
        b.put_samples(0, Y, np.repeat(np.repeat(U, 2, 0), 2, 1), np.repeat(np.repeat(V, 2, 0), 2, 1))
        da, db = (FK.pix_layout(1, W, Hh, fmt, aligned=True, fill=FK.GUARD) for _ in range(2))
        assert (YX.host_to_frames(L, a, da) == YX.host_to_frames(L, b, db)).all(), (W, Hh)


def test_the_low_bits_of_p010_are_ignored_and_written_as_zero(L):
    for i, (W, Hh) in enumerate(YX.SIZES):
        m, r = YX.variant(i)
        a = YX.YuvEx(2, W, Hh, "nv12", 10, aligned=bool(i % 2), seed=W, matrix=m, rng=r)
        b = YX.YuvEx(2, W, Hh, "nv12", 10, aligned=bool(i % 2), matrix=m, rng=r)
        for f in range(2):
            for k in range(2):
                assert (a.words(f, k) & 63).any()
                b.put_words(f, k, a.words(f, k) & ~63)
        dst = FK.pix_layout(2, W, Hh, "bgr", aligned=True, fill=FK.GUARD)
        assert (YX.host_to_frames(L, a, dst) == YX.host_to_frames(L, b, dst)).all()
        out = YX.host_to_yuv(L, FK.pix_layout(2, W, Hh, "bgr", aligned=True, seed=W), b)
        for f in range(2):
            for k in range(2):
                w = b.words(f, k, out)
                assert (w & 63 == 0).all() and (w >> 6).max() > 512


@pytest.mark.parametrize("m", MATS)
def test_p016_of_shifted_bytes_is_the_8_bit_conversion_within_1(L, m):
    """a P016 frame whose words are s << 8, limited range: every channel within 1 level of the 8-bit conversion of s"""
    worst = 0
    for W, Hh in YX.SIZES:
        a = YX.YuvEx(1, W, Hh, "nv12", 8, aligned=True, seed=W + 3, matrix=m)
        b = YX.YuvEx(1, W, Hh, "nv12", 16, aligned=True, matrix=m)
        for k in range(2):
            b.put_words(0, k, a.plane_view(0, k).astype(np.int64) << 8)
        da, db = (FK.pix_layout(1, W, Hh, "bgr", aligned=True, fill=FK.GUARD) for _ in range(2))
        d = np.abs(YX.host_to_frames(L, a, da).astype(int) - YX.host_to_frames(L, b, db).astype(int))
        worst = max(worst, int(d.max()))
    print("%s: P016 of s << 8 is at most %d from the 8-bit conversion" % (m, worst))
    assert worst <= 1


# ---- 5. the round trip ------------------------------------------------------------------------------------------------------------------

def test_the_round_trip_of_constant_blocks_is_no_worse_than_the_8_bit_bt601_path(L):
    """Constant 2 x 2 blocks of 2^21 random colours (seed 5) and of every combination of the channels' edges go colour -> YUV ->
    colour, per table and depth.  The worst channel error of the 8-bit BT.601 limited path, measured here, is the bar of every
    other table.  Measured: 2 for the yardstick and for every limited-range table at 8 bits, 1 for every full-range table at 8
    bits, 0 for every table at 10, 12 and 16 bits."""
    rng = np.random.default_rng(5)
    e = np.array(edge_values(255))
    Bc, Gc, Rc = np.meshgrid(e, e, e, indexing="ij")
    bgr = np.concatenate([np.stack([Bc.ravel(), Gc.ravel(), Rc.ravel()], 1), rng.integers(0, 256, (1 << 21, 3))]).astype(np.uint8)

    def worst(t):
        back = host_bgr(L, t, host_yuv(L, t, bgr, 2))
        return int(np.abs(back - bgr.astype(np.int64)).max())

    bar = worst(("bt601", "limited", 8))
    print("the 8-bit BT.601 limited round trip moves a channel by at most %d" % bar)
    got = {t: worst(t) for t in TABLES}
    for t, w in got.items():
        print("%s: at most %d" % (tid(t), w))
    assert all(w <= bar for w in got.values()), got


# ---- 6. refusals of the host call -----------------------------------------------------------------------------------------------------------

def test_refusals_of_the_host_call(L):
    W, Hh, n = 64, 32, 2
    pix = np.full(n * 4 * W * Hh + 64, FK.GUARD, np.uint8)
    yuv = np.full(n * 6 * W * Hh + 64, 77, np.uint8)
    pp, yp = pix.ctypes.data, yuv.ctypes.data
    assert yp % 2 == 0
    span = (2 ** 31) // (Hh - 1) + 1       # a pitch with which the rows of a plane span more than 2^31 - 1 bytes
    span_c = (2 ** 31) // (Hh // 2 - 1) + 1

    def call(to_frames, **kw):
        a = dict(layout=0, matrix=0, range=0, bits=8, y=yp, c0=yp + 2 * W * Hh, c1=yp + 4 * W * Hh, yp=W, cp=W, fs=6 * W * Hh, pix=pp, rs=3 * W,
                 w=W, h=Hh, n=n, fmt=0, lw=W, lh=Hh)
        a.update(kw)
        st = YX.FramesEx(a["layout"], a["matrix"], a["range"], a["bits"], a["y"], a["c0"], a["c1"], a["yp"], a["cp"], a["fs"])
        ref = C.addressof(st) if a.get("st", True) else None
        pfs = a.get("pfs", a["rs"] * a["h"])
        if to_frames:
            return L.yuv_ex_to_frames_emul(ref, a["pix"], a["rs"], pfs, a["w"], a["h"], a["n"], a["fmt"], a["lw"], a["lh"])
        return L.yuv_ex_from_frames_emul(a["pix"], a["rs"], pfs, ref, a["w"], a["h"], a["n"], a["fmt"], a["lw"], a["lh"])

    p010 = dict(bits=10, yp=2 * W, cp=2 * W)
    cases = [
        (dict(st=False), YX.BAD_NO_FRAMES), (dict(pix=None), YX.BAD_NO_FRAMES),
        # everything the existing calls refuse
        (dict(y=None), YX.BAD_NO_PLANE), (dict(c0=None), YX.BAD_NO_PLANE), (dict(layout=1, cp=W // 2, c1=None), YX.BAD_NO_PLANE),
        (dict(layout=1, cp=W // 2, c0=None), YX.BAD_NO_PLANE), (dict(layout=4, c0=None), YX.BAD_NO_PLANE), (dict(layout=5, c1=None), YX.BAD_NO_PLANE),
        (dict(layout=6), YX.BAD_UNKNOWN), (dict(layout=-1), YX.BAD_UNKNOWN), (dict(matrix=3), YX.BAD_UNKNOWN), (dict(matrix=-1), YX.BAD_UNKNOWN),
        (dict(fmt=5), YX.BAD_UNKNOWN), (dict(fmt=-1), YX.BAD_UNKNOWN),
        (dict(w=W - 1), YX.BAD_ODD_SIDE), (dict(layout=2, yp=2 * W, w=W - 3), YX.BAD_ODD_SIDE), (dict(h=Hh - 1), YX.BAD_ODD_SIDE),
        (dict(layout=1, cp=W // 2, h=Hh - 1), YX.BAD_ODD_SIDE), (dict(layout=4, h=Hh - 1), YX.BAD_ODD_SIDE), (dict(layout=4, w=W - 1), YX.BAD_ODD_SIDE),
        (dict(w=W + 2), YX.BAD_SIDE), (dict(h=Hh + 2), YX.BAD_SIDE), (dict(w=0), YX.BAD_SIDE), (dict(h=0), YX.BAD_SIDE), (dict(n=0), YX.BAD_SIDE),
        (dict(n=-1), YX.BAD_SIDE), (dict(layout=5, w=W + 1), YX.BAD_SIDE),
        (dict(yp=W - 1), YX.BAD_PITCH), (dict(cp=W - 1), YX.BAD_PITCH), (dict(layout=1, cp=W // 2 - 1), YX.BAD_PITCH),
        (dict(layout=2, yp=2 * W - 1), YX.BAD_PITCH), (dict(layout=3, yp=2 * W - 1), YX.BAD_PITCH), (dict(layout=5, cp=W - 1), YX.BAD_PITCH),
        (dict(layout=4, cp=W - 1), YX.BAD_PITCH), (dict(p010, yp=2 * W - 2), YX.BAD_PITCH), (dict(p010, cp=2 * W - 2), YX.BAD_PITCH),
        (dict(rs=3 * W - 1), YX.BAD_ROW_STRIDE), (dict(fmt=2, rs=4 * W - 1), YX.BAD_ROW_STRIDE), (dict(fmt=4, rs=W - 1), YX.BAD_ROW_STRIDE),
        (dict(yp=span, n=1), YX.BAD_SPAN), (dict(cp=span_c, n=1), YX.BAD_SPAN), (dict(layout=1, cp=span_c, n=1), YX.BAD_SPAN),
        (dict(layout=2, yp=span, n=1), YX.BAD_SPAN), (dict(layout=5, cp=span, n=1), YX.BAD_SPAN), (dict(rs=span, pfs=3 * W * Hh, n=1), YX.BAD_SPAN),
        (dict(pix=yp), YX.BAD_OVERLAP), (dict(pix=yp + 6 * W * Hh * n - 4 * W * Hh - 1), YX.BAD_OVERLAP), (dict(pix=yp + W * Hh), YX.BAD_OVERLAP),
        (dict(y=pp + 1), YX.BAD_OVERLAP), (dict(c0=pp + 3 * W * Hh * n - 1), YX.BAD_OVERLAP), (dict(layout=1, cp=W // 2, c1=pp), YX.BAD_OVERLAP),
        (dict(layout=5, c1=pp + 8), YX.BAD_OVERLAP), (dict(layout=3, yp=2 * W, y=pp + 3 * W * Hh * n - 1), YX.BAD_OVERLAP),
        # the range and the depth
        (dict(range=2), YX.BAD_UNKNOWN), (dict(range=-1), YX.BAD_UNKNOWN), (dict(bits=9), YX.BAD_UNKNOWN), (dict(bits=0), YX.BAD_UNKNOWN),
        (dict(bits=14), YX.BAD_UNKNOWN), (dict(bits=17), YX.BAD_UNKNOWN), (dict(bits=-8), YX.BAD_UNKNOWN),
        # more than 8 bits with another layout
        *[(dict(p010, layout=lay, bits=b), YX.BAD_DEPTH_LAYOUT) for lay in (1, 2, 3, 4, 5) for b in (10, 12, 16)],
        # an odd 16-bit pitch (and address, and frame stride)
        (dict(p010, yp=2 * W + 1), YX.BAD_ODD_WORDS), (dict(p010, cp=2 * W + 1), YX.BAD_ODD_WORDS), (dict(p010, bits=16, yp=2 * W + 3), YX.BAD_ODD_WORDS),
        (dict(p010, y=yp + 1), YX.BAD_ODD_WORDS), (dict(p010, c0=yp + 2 * W * Hh + 1), YX.BAD_ODD_WORDS), (dict(p010, fs=6 * W * Hh + 1), YX.BAD_ODD_WORDS),
    ]
    before = yuv.copy()
    for to_frames in (True, False):
        for kw, why in cases:
            assert call(to_frames, **kw) == why, (to_frames, kw)
    assert (pix == FK.GUARD).all() and (yuv == before).all()   # nothing was written on either side
    # the context's size limit is the call's: a frame above it is refused, the frame at it is not
    assert call(True, lw=W - 2) == YX.BAD_SIDE and call(False, lh=Hh - 2) == YX.BAD_SIDE and call(True, layout=5, w=33, h=31, lw=32) == YX.BAD_SIDE
    # what is no fault: an odd height with 4:2:2, odd sides with I444, an odd 8-bit pitch, a plane pointer the layout does not use
    assert call(True, layout=2, yp=2 * W, h=Hh - 1, c0=None, c1=None) == 0
    assert call(True, layout=5, w=W - 1, h=Hh - 1) == 0 and call(True, yp=W + 1, cp=W + 3) == 0 and call(True, c1=None) == 0
    assert call(True, **p010) == 0 and call(False, **dict(p010, bits=16)) == 0 and call(False, layout=4, range=1, matrix=2) == 0
    assert (pix != FK.GUARD).any()


# ---- 7. the chain on the oracle ---------------------------------------------------------------------------------------------------------

PATHS = [("p010 bt2020 limited", "nv12", 10, "bt2020", "limited"), ("nv12 bt709 full", "nv12", 8, "bt709", "full"),
         ("i444 bt601 full", "i444", 8, "bt601", "full"), ("nv21 bt601 limited", "nv21", 8, "bt601", "limited")]
MATCH_PX = 8.0   # a record is recovered by a record of the same template whose corners lie this near (markers lie 40 px and more apart)


def round_trip_ex(L, bgr, layout, bits, m, r):
    Hh, W = bgr.shape[:2]
    src = FK.pix_layout(1, W, Hh, "bgr", aligned=True)
    src.view(0)[...] = bgr
    yuv = YX.YuvEx(1, W, Hh, layout, bits, aligned=True, matrix=m, rng=r)
    back = FK.pix_layout(1, W, Hh, "bgr", aligned=True, fill=FK.GUARD)
    return np.ascontiguousarray(back.view(0, YX.host_to_frames(L, yuv, back, buf=YX.host_to_yuv(L, src, yuv))))


def round_trip_old(LY, bgr):
    Hh, W = bgr.shape[:2]
    src = FK.pix_layout(1, W, Hh, "bgr", aligned=True)
    src.view(0)[...] = bgr
    yuv = YC.Yuv(1, W, Hh, "nv12", aligned=True)
    back = FK.pix_layout(1, W, Hh, "bgr", aligned=True, fill=FK.GUARD)
    return np.ascontiguousarray(back.view(0, YC.host_to_frames(LY, yuv, "bt601", back, buf=YC.host_to_yuv(LY, src, "bt601", yuv))))


def recovered(found, truth):
    """for every record of truth: the corner distance of the nearest found record with its template, or None beyond MATCH_PX"""
    out = []
    for t in truth:
        d = [BC.corner_set_distance(m.square, t.square) for m in found if m.templateId == t.templateId]
        out.append(min(d) if d and min(d) <= MATCH_PX else None)
    return out


def test_the_chain_on_the_oracle(L, LY):
    """The eight scenes of levels_chain.chain_scenes() (14 records on the originals) go frames -> YUV -> frames on the host core:
    through P010 BT.2020 limited, NV12 BT.709 full, I444 BT.601 full, NV21 BT.601 limited, and through the existing NV12 BT.601
    limited path, the yardstick.  On every scene a new path recovers every record the yardstick recovers, with the same template,
    its corners within the yardstick's worst corner distance on that scene plus 1 px.  Measured: the yardstick and each of the four
    paths recover 14 of 14 records; corners move by 0 px, but for NV21 on scene 640x480-3: 2 px, where the yardstick's bar is 3 px."""
    tpls = H.oracle_templates()
    counts = {"yardstick": 0, **{p[0]: 0 for p in PATHS}}
    total = 0
    for name, bgr in LC.chain_scenes():
        cam = H.oracle_camera(bgr.shape[1], bgr.shape[0])
        truth = H.oracle_registration(bgr, tpls, cam)[0]
        total += len(truth)
        yard = recovered(H.oracle_registration(round_trip_old(LY, bgr), tpls, cam)[0], truth)
        counts["yardstick"] += sum(d is not None for d in yard)
        bar = max([d for d in yard if d is not None] or [0.0]) + 1.0
        for label, layout, bits, m, r in PATHS:
            got = recovered(H.oracle_registration(round_trip_ex(L, bgr, layout, bits, m, r), tpls, cam)[0], truth)
            counts[label] += sum(d is not None for d in got)
            print("%-12s %-20s %d of %d records (yardstick %d), corners within %.2f px (bar %.2f)" % (
                name, label, sum(d is not None for d in got), len(truth), sum(d is not None for d in yard),
                max([d for d in got if d is not None] or [0.0]), bar))
            for k, (dy, dg) in enumerate(zip(yard, got)):
                if dy is not None:
                    assert dg is not None and dg <= bar, (name, label, k, dy, dg)
    print("records recovered of %d: %r" % (total, counts))
    assert total == 14 and counts["yardstick"] >= 1


# ---- 8. the sanitizers ----------------------------------------------------------------------------------------------------------------------

def test_the_emulation_is_clean_under_the_sanitizers():
    """tests/emul/yuv_ex_emul.cpp with its own main -- the layout x depth x format sweep on heap blocks of exactly the bytes a
    conversion may touch, sides from 1 up to a single row of 1027 pixels -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own"""
    run_sanitized("yuv_ex_emul", "YUV_EX_EMUL_MAIN", "430 cases, 0 bad", timeout=300)


# ---- 9. the ABI ---------------------------------------------------------------------------------------------------------------------------

def test_the_abi_surface():
    import subprocess
    import opencv_ar_amd as oa
    header = open(os.path.join(H.ROOT, "include", "ocvar_hip.h")).read()
    lib = H._build(os.path.join(H.PKG, "lib", "libocvar_hip.so"), "lib/libocvar_hip.so", H.PKG)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for sym in ("ocvar_hip_yuv_to_frames_ex", "ocvar_hip_frames_to_yuv_ex"):
        assert re.search(r"\bint %s\(" % sym, header) and sym in oa.HIP_SYMBOLS and re.search(r" T %s$" % sym, exported, re.M), sym
    # the struct: 56 bytes, the header's field order
    m = re.search(r"typedef struct \{([^}]*)\} OcvarYuvFramesEx;", header)
    names = [w for w in re.findall(r"[a-z_0-9]+", m.group(1)) if w not in ("int", "void", "size_t")]
    assert names == [f[0] for f in oa.YuvFramesEx._fields_] == [f[0] for f in YX.FramesEx._fields_]
    assert C.sizeof(oa.YuvFramesEx) == C.sizeof(YX.FramesEx) == 56 and "/* 56 bytes */" in header
    assert [(f[0], f[1]) for f in oa.YuvFramesEx._fields_] == [(f[0], f[1]) for f in YX.FramesEx._fields_]
    for name, table, prefix in (("nv21", oa.YUV_EX_LAYOUTS, "OCVAR_YUV_NV21"), ("i444", oa.YUV_EX_LAYOUTS, "OCVAR_YUV_I444"),
                                ("bt2020", oa.YUV_EX_MATRICES, "OCVAR_YUV_BT2020"), ("limited", oa.YUV_RANGES, "OCVAR_YUV_LIMITED"),
                                ("full", oa.YUV_RANGES, "OCVAR_YUV_FULL")):
        assert int(re.search(r"%s = (\d+)" % prefix, header).group(1)) == table[name]
    assert oa.YUV_EX_LAYOUTS == YX.LAYOUTS and oa.YUV_EX_MATRICES == YX.MATRICES and oa.YUV_RANGES == YX.RANGES
    # the existing descriptor keeps refusing what the old ABI refuses
    for kw in (dict(layout="nv21"), dict(layout="i444"), dict(layout=4), dict(layout="nv12", matrix="bt2020"), dict(layout="nv12", matrix=2)):
        with pytest.raises(ValueError):
            oa.YuvFrames.from_surface(4096, 64, 32, **kw)
    # the Python checks raise for what the ABI refuses
    for kw in (dict(layout="nv42"), dict(layout=6), dict(layout="nv12", matrix="bt470"), dict(layout="nv12", range="tv"), dict(layout="nv12", range=2),
               dict(layout="nv12", bits=9), dict(layout="nv12", bits=True), dict(layout="i420", bits=10), dict(layout="nv21", bits=16),
               dict(layout="i444", bits=12), dict(layout="yuyv", bits=10), dict(layout="nv12", bits=10, pitch=129), dict(layout="nv12", height=31),
               dict(layout="i420", pitch=65)):
        a = dict(ptr=4096, width=64, height=32)
        a.update(kw)
        with pytest.raises(ValueError):
            oa.YuvFramesEx.from_surface(**a)
    with pytest.raises(ValueError):
        oa.YuvFramesEx.from_surface(4097, 64, 32, "nv12", bits=10)
    # what from_surface lays out
    s = oa.YuvFramesEx.from_surface(4096, 64, 32, "nv12", bits=10, matrix="bt2020", range="full")
    assert (s.layout, s.matrix, s.range, s.bits, s.y, s.c0, s.c1, s.y_pitch, s.c_pitch, s.frame_stride) == (0, 2, 1, 10, 4096, 4096 + 128 * 32, None, 128, 128, 128 * 48)
    s = oa.YuvFramesEx.from_surface(4096, 63, 31, "i444", pitch=64)
    assert (s.layout, s.bits, s.y, s.c0, s.c1, s.y_pitch, s.c_pitch, s.frame_stride) == (5, 8, 4096, 4096 + 64 * 31, 4096 + 128 * 31, 64, 64, 192 * 31)
    s = oa.YuvFramesEx.from_surface(4096, 64, 32, "nv21")
    assert (s.layout, s.c0, s.c1, s.c_pitch, s.frame_stride) == (4, 4096 + 64 * 32, None, 64, 64 * 48)

    # Detector.yuv_to_frames and frames_to_yuv go to the entry point of the descriptor's type
    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append(name) or 0

    calls = []
    det = oa.Detector.__new__(oa.Detector)
    det._lib, det._ctx = Lib(), None
    det.input_format = 0
    old, new = oa.YuvFrames.from_surface(4096, 64, 32, "nv12"), oa.YuvFramesEx.from_surface(4096, 64, 32, "nv12")
    det.yuv_to_frames(old, 1 << 20, 64, 32, 1)
    det.yuv_to_frames(new, 1 << 20, 64, 32, 1)
    det.frames_to_yuv(1 << 20, old, 64, 32, 1)
    det.frames_to_yuv(1 << 20, new, 64, 32, 1)
    assert calls == ["ocvar_hip_yuv_to_frames", "ocvar_hip_yuv_to_frames_ex", "ocvar_hip_frames_to_yuv", "ocvar_hip_frames_to_yuv_ex"]
    with pytest.raises(TypeError):
        det.yuv_to_frames(object(), 1 << 20, 64, 32, 1)

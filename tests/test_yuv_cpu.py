"""The YUV conversion core (opencv-ar_amd/csrc/yuv_core.h) on the host (tests/yuv_chain.py builds it): the three formulas on all
2^24 inputs against a numpy restatement and against the float64 matrices, what they promise (greys stay grey, the limited range,
the round trip), and the two frame loops on every layout, format and border case with guard bytes around every row, plane and
frame.  tests/test_gpu_yuv.py holds the kernels to this build byte for byte."""
import subprocess

import numpy as np
import pytest

import frame_kit as FK
import overlay_chain as OC
import yuv_chain as YC
from helpers import P
from hostbuild import run_sanitized

MATS = ["bt601", "bt709"]
N24 = 1 << 24


@pytest.fixture(scope="module")
def L():
    return YC.build_emul()


@pytest.fixture(scope="module")
def to_colour(L):
    """matrix -> [2^24, 3] B G R of the host core, index (Y << 16) | (U << 8) | V; computed once"""
    out = {}
    for m in MATS:
        a = np.zeros((N24, 3), np.uint8)
        L.yuv_to_bgr_all_emul(YC.MATRICES[m], P(a))
        a.setflags(write=False)
        out[m] = a
    return out


@pytest.fixture(scope="module")
def to_yuv(L):
    """(matrix, log2n) -> [2^24, 3] Y U V of the host core for constant blocks, index (B << 16) | (G << 8) | R; computed once"""
    out = {}
    for m in MATS:
        for log2n in (1, 2):
            a = np.zeros((N24, 3), np.uint8)
            assert L.bgr_to_yuv_all_emul(YC.MATRICES[m], log2n, P(a)) == 0   # (nothing was cut by the cast to a byte)
            a.setflags(write=False)
            out[m, log2n] = a
    return out


def triples():
    """the three bytes of every index 0 .. 2^24 - 1, most significant first, as int64"""
    i = np.arange(N24, dtype=np.int64)
    return i >> 16, (i >> 8) & 255, i & 255


def test_the_tables_are_the_stated_ones(L):
    for m in MATS:
        got = np.zeros(14, np.int32)
        L.yuv_coef_emul(YC.MATRICES[m], P(got))
        assert dict(zip(YC.COEF_NAMES, got.tolist())) == YC.COEF[m]
        assert np.abs(got).max() < 1 << 23   # (the 24-bit multiplier of the kernels is exact)
    # BT.709: round(x * 2^20) of the matrix with Kr = 0.2126, Kb = 0.0722 and the scales 255/219 and 255/224
    assert {k: int(np.floor(v * 2 ** 20 + 0.5)) for k, v in float_matrix("bt709").items()} == YC.COEF["bt709"]


def float_matrix(m):
    """the float64 matrix a table stands for: BT.601 the three-digit one, BT.709 from Kr and Kb"""
    if m == "bt601":
        return dict(cy=1.164, cub=2.018, cug=-0.391, cvg=-0.813, cvr=1.596, ry=0.257, gy=0.504, by=0.098, ru=-0.148, gu=-0.291, bu=0.439,
                    rv=0.439, gv=-0.368, bv=-0.071)
    kr, kb = 0.2126, 0.0722
    kg = 1 - kr - kb
    sy, sc = 255.0 / 219.0, 255.0 / 224.0
    return dict(cy=sy, cvr=2 * (1 - kr) * sc, cub=2 * (1 - kb) * sc, cug=-2 * kb * (1 - kb) / kg * sc, cvg=-2 * kr * (1 - kr) / kg * sc,
                ry=kr / sy, gy=kg / sy, by=kb / sy, ru=-kr / (2 * (1 - kb)) / sc, gu=-kg / (2 * (1 - kb)) / sc, bu=0.5 / sc,
                rv=0.5 / sc, gv=-kg / (2 * (1 - kr)) / sc, bv=-kb / (2 * (1 - kr)) / sc)


@pytest.mark.parametrize("m", MATS)
def test_yuv_to_colour_on_every_triple(to_colour, m):
    Y, U, V = triples()
    B, G, R = YC.np_yuv_to_bgr(m, Y, U, V)
    got = to_colour[m]
    assert (got[:, 0] == B).all() and (got[:, 1] == G).all() and (got[:, 2] == R).all()
    # the float64 matrix (with the same max(Y - 16, 0)), rounded half up and clamped: at most 1 away
    f = float_matrix(m)
    y = np.maximum(Y - 16, 0) * f["cy"]
    for c, want in ((2, y + f["cvr"] * (V - 128)), (1, y + f["cvg"] * (V - 128) + f["cug"] * (U - 128)), (0, y + f["cub"] * (U - 128))):
        d = np.abs(got[:, c].astype(np.int64) - np.clip(np.floor(want + 0.5), 0, 255).astype(np.int64)).max()
        print("%s, channel %s: at most %d from the float64 matrix" % (m, "BGR"[c], d))
        assert d <= 1
    # U = V = 128 gives B = G = R; Y <= 16 gives 0 and Y >= 235 gives 255 there
    grey = got[(U == 128) & (V == 128)]
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all() and len(grey) == 256
    assert (grey[:17] == 0).all() and (grey[235:] == 255).all() and (np.diff(grey[:, 0].astype(int)) >= 0).all()


@pytest.mark.parametrize("m", MATS)
def test_colour_to_yuv_on_every_colour(to_yuv, m):
    B, G, R = triples()
    f = float_matrix(m)
    for log2n in (1, 2):
        got = to_yuv[m, log2n]
        assert (got[:, 0] == YC.np_luma(m, B, G, R)).all()
        U, V = YC.np_chroma(m, B << log2n, G << log2n, R << log2n, log2n)
        assert (got[:, 1] == U).all() and (got[:, 2] == V).all()
        # the limited range, and a grey pixel has no colour
        assert got[:, 0].min() == 16 and got[:, 0].max() == 235
        assert got[:, 1].min() == 16 and got[:, 1].max() == 240 and got[:, 2].min() == 16 and got[:, 2].max() == 240
        grey = got[(B == G) & (G == R)]
        assert (grey[:, 1:] == 128).all() and len(grey) == 256
        # the float64 matrix, rounded half up: at most 1 away
        for c, want in ((0, f["ry"] * R + f["gy"] * G + f["by"] * B + 16), (1, f["ru"] * R + f["gu"] * G + f["bu"] * B + 128),
                        (2, f["rv"] * R + f["gv"] * G + f["bv"] * B + 128)):
            d = np.abs(got[:, c].astype(np.int64) - np.clip(np.floor(want + 0.5), 0, 255).astype(np.int64)).max()
            print("%s, %d pixels per sample, %s: at most %d from the float64 matrix" % (m, 1 << log2n, "YUV"[c], d))
            assert d <= 1
    assert (to_yuv[m, 1] == to_yuv[m, 2]).all()   # (a constant block's chroma does not depend on its size)


@pytest.mark.parametrize("m", MATS)
def test_the_round_trip_of_constant_blocks(to_colour, to_yuv, m):
    """colour -> YUV -> colour returns every channel within 2, over all 2^24 colours"""
    B, G, R = triples()
    yuv = to_yuv[m, 2].astype(np.int64)
    back = to_colour[m][(yuv[:, 0] << 16) | (yuv[:, 1] << 8) | yuv[:, 2]].astype(np.int64)
    worst = [int(np.abs(back[:, c] - ch).max()) for c, ch in enumerate((B, G, R))]
    print("%s: the round trip moves B G R by at most %s" % (m, worst))
    assert max(worst) <= 2


@pytest.mark.parametrize("m", MATS)
@pytest.mark.parametrize("log2n", [1, 2])
def test_chroma_of_mixed_blocks(L, m, log2n):
    """blocks of random pixels, of extreme ones and of one bright pixel among dark ones"""
    rng = np.random.default_rng(log2n)
    px = rng.integers(0, 256, (200000, 1 << log2n, 3))
    px[:50000] = rng.integers(0, 2, (50000, 1 << log2n, 3)) * 255
    px[50000:60000, 1:] = 0
    sums = np.ascontiguousarray(px.sum(1), np.int32)
    got = np.zeros((len(sums), 2), np.uint8)
    L.yuv_chroma_emul(YC.MATRICES[m], log2n, P(sums), len(sums), P(got))
    U, V = YC.np_chroma(m, sums[:, 0], sums[:, 1], sums[:, 2], log2n)
    assert (got[:, 0] == U).all() and (got[:, 1] == V).all()
    assert got.min() == 16 and got.max() == 240 and len(np.unique(got)) > 100   # (the extremes are among them, and much between)


# ---- the frame loops ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(YC.LAYOUTS))
@pytest.mark.parametrize("fmt", FK.FMTS)
def test_yuv_to_frames_on_every_layout_format_and_border(L, layout, fmt):
    """an odd leading offset, row padding, a gap between the planes and between the frames; two frames; both tables"""
    for i, (W, Hh) in enumerate(YC.SIZES):
        m = MATS[i % 2]
        yuv = YC.Yuv(2, W, Hh, layout, aligned=False, seed=W + Hh)
        dst = FK.pix_layout(2, W, Hh, fmt, aligned=False, fill=FK.GUARD)
        out = YC.host_to_frames(L, yuv, m, dst)
        assert (out[~dst.pixel_mask()] == FK.GUARD).all(), (W, Hh)
        for f in range(2):
            want = YC.np_frame_to_pixels(m, fmt, *yuv.samples(f))
            assert (dst.view(f, out) == want).all(), (W, Hh, f)
            if dst.bpp == 4:
                assert (dst.view(f, out)[..., 3] == 255).all()
        if fmt == "gray":   # the library's grey of the BGR target, byte for byte
            bgr = FK.pix_layout(2, W, Hh, "bgr", aligned=True, fill=FK.GUARD)
            ob = YC.host_to_frames(L, yuv, m, bgr)
            for f in range(2):
                b = bgr.view(f, ob).astype(np.int64)
                assert (dst.view(f, out)[..., 0] == OC.grey_of(b[..., 0], b[..., 1], b[..., 2])).all()


@pytest.mark.parametrize("layout", list(YC.LAYOUTS))
@pytest.mark.parametrize("fmt", FK.FMTS)
def test_frames_to_yuv_on_every_layout_format_and_border(L, layout, fmt):
    for i, (W, Hh) in enumerate(YC.SIZES):
        m = MATS[(i + 1) % 2]
        src = FK.pix_layout(2, W, Hh, fmt, aligned=False, seed=W * Hh)
        yuv = YC.Yuv(2, W, Hh, layout, aligned=False)
        out = YC.host_to_yuv(L, src, m, yuv)
        assert (out[~yuv.sample_mask()] == FK.GUARD).all(), (W, Hh)
        for f in range(2):
            want = YC.np_pixels_to_frame(m, fmt, src.view(f), yuv.s420)
            for got_plane, want_plane in zip(yuv.samples(f, out), want):
                assert (got_plane == want_plane).all(), (W, Hh, f)
        if src.bpp == 4:   # byte 3 of a source pixel is ignored
            other = src.buf.copy()
            for f in range(2):
                src.view(f, other)[..., 3] ^= 0x5A
            assert (YC.host_to_yuv(L, src, m, yuv, buf=other) == out).all()


@pytest.mark.parametrize("fmt", ["bgr", "rgba", "gray"])
def test_the_layouts_of_a_subsampling_hold_the_same_samples(L, fmt):
    for W, Hh in YC.SIZES:
        src = FK.pix_layout(1, W, Hh, fmt, aligned=True, seed=W)
        for a, b in (("nv12", "i420"), ("yuyv", "uyvy")):
            ya, yb = YC.Yuv(1, W, Hh, a), YC.Yuv(1, W, Hh, b, aligned=True)
            sa, sb = ya.samples(0, YC.host_to_yuv(L, src, "bt601", ya)), yb.samples(0, YC.host_to_yuv(L, src, "bt601", yb))
            assert all((p == q).all() for p, q in zip(sa, sb)), (W, Hh, a, b)
            # and back: the same pixels from either layout
            da, db = (FK.pix_layout(1, W, Hh, fmt, aligned=False, fill=FK.GUARD) for _ in range(2))
            ya.put_samples(0, *sa)
            yb.put_samples(0, *sb)
            assert (YC.host_to_frames(L, ya, "bt601", da) == YC.host_to_frames(L, yb, "bt601", db)).all()


def test_the_shipped_kernels_hold_no_packed_shift_saturate(tmp_path):
    """yuv_core.h clamps before it shifts so that the compiler does not build v_ashr_pk_u8_i32 (whose upper result half it takes
    for zero, and the MI355X left as it was: one wrong byte per lane in the first device run).  Which instruction it builds is the
    compiler's choice, so it is checked in the binary, as tests/test_code_object.py does for the wide stores."""
    import os
    import sys
    import helpers as H
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import check_store_hazard as CSH
    lib = H._build(os.path.join(H.PKG, "lib", "libocvar_hip.so"), "lib/libocvar_hip.so", H.PKG)
    seen = 0
    for co in CSH.code_objects(lib, str(tmp_path)):
        listing = subprocess.run([os.path.join(CSH.LLVM, "llvm-objdump"), "-d", "-C", "--no-show-raw-insn", "--mcpu=" + CSH.ARCH, co],
                                 check=True, capture_output=True, text=True).stdout
        seen += listing.count("yuv_to_frames_kernel<") + listing.count("frames_to_yuv_kernel<")
        assert "v_ashr_pk_" not in listing, CSH.compiler_version()
    assert seen >= 24   # (the listing held the kernels: 2 directions x 3 pixel sizes x 2 alignments x 2 subsamplings)


def test_the_emulation_is_clean_under_the_sanitizers():
    """tests/emul/yuv_emul.cpp with its own main -- the layout sweep on heap blocks of exactly the bytes a conversion may touch --
    built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own"""
    run_sanitized("yuv_emul", "YUV_EMUL_MAIN", "360 cases, 0 bad", timeout=300)

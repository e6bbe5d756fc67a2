"""The address arithmetic of the kernels over the WHOLE range of sizes the C ABI admits (contexts of 16 .. 32767 pixels each way,
any row_stride that fits an int), against plain integers: the bounds that so far lived in comments of hd.h.  The device builds
tile offsets and the row division with the 24-bit multiplier; the host build multiplies in 32 bits, so the tests here also model
__umul24 / __mul24 and require them to be exact for every operand pair the call sites can form.

The GPU side of the same limits is tests/test_gpu_geometry_limits.py."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from helpers import P
from hostbuild import host_core

MAX_SIDE = 32767                          # api.hip::create_impl
NS_MAX = ((MAX_SIDE & ~1) + 15) & ~15     # 32768 columns of the bit plane
SH_MAX = MAX_SIDE & ~1                    # 32766 rows
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def G():
    L = host_core("geometry_emul")
    L.geo_div14.restype = C.c_uint
    L.geo_div14.argtypes = [C.c_uint]
    L.geo_div14_range.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
    L.geo_plane_bytes.restype = C.c_longlong
    L.geo_tile_off.restype = C.c_uint
    L.geo_tile_off.argtypes = [C.c_uint, C.c_uint, C.c_int]
    L.geo_win_offs.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.geo_frame_src_addressable.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int]
    L.geo_march_src_bytes.restype = C.c_longlong
    return L


def umul24(a, b):
    """v_mul_u32_u24: the low 32 bits of the product of the operands' low 24 bits"""
    return ((a & 0xffffff) * (b & 0xffffff)) & 0xffffffff


def mul24(a, b):
    """v_mul_i32_i24: the operands' low 24 bits sign-extended, the low 32 bits of their product as a signed int"""
    sx = lambda v: ((v & 0xffffff) ^ 0x800000) - 0x800000
    p = (sx(a) * sx(b)) & 0xffffffff
    return p - (1 << 32) if p & 0x80000000 else p


def test_div14_is_exact_up_to_the_bound_its_comment_claims(G):
    """hd.h::div14(y) = (y * 37450) >> 19 is y // 14 for every row a context can have (0 .. 32767) and up to 43689, the bound the
    comment states; the first y it gets wrong is 43693 (the next one of remainder 13), so the stated bound is the real one."""
    n = 43690
    got = np.zeros(n, np.uint32)
    G.geo_div14_range(0, n, P(got))
    want = [y // 14 for y in range(n)]
    assert got.tolist() == want
    assert G.geo_div14(MAX_SIDE) == MAX_SIDE // 14 == 2340
    first_wrong = next(y for y in range(n, 2 * n) if (y * 37450) >> 19 != y // 14)
    assert first_wrong == 43693 and G.geo_div14(first_wrong) == 43693 // 14 + 1


def test_the_24_bit_multiplier_is_exact_at_every_call_site(G):
    """__umul24 (modelled: low 24 bits of each operand, low 32 bits of the product) equals the exact product for every operand pair
    of its three call sites -- nbr_tile_off / nbr_win_off_xy: tile row ty <= 2340 times tiles per row nt <= 2048; div14: y <= 32767
    (and to 43689) times 37450 -- and __mul24 equals it for trace_core.h::mul_small's dy * ns, dy in {-1, 0, 1}."""
    ty = np.arange(0, 2341, dtype=np.int64)[:, None]
    nt = np.arange(0, 2049, dtype=np.int64)[None, :]
    exact = ty * nt
    assert np.array_equal(((ty & 0xffffff) * (nt & 0xffffff)) & 0xffffffff, exact)
    assert int(exact.max()) == 2340 * 2048 < 2**24 * 2**8
    for y in range(43690):
        assert umul24(y, 37450) == y * 37450
    for ns in (16, 608, 3840, NS_MAX):
        for d in (-1, 0, 1):
            assert mul24(d, ns) == d * ns == G.geo_mul_small(d, ns)
    # the model itself: it does differ from the product once an operand passes 24 bits or the product 32
    assert umul24(1 << 24, 3) == 0 and umul24(0xffffff, 0xffffff) != 0xffffff * 0xffffff and mul24(0x800000, 1) == -0x800000


@pytest.mark.parametrize("ns", [16, 608, 3840, NS_MAX])
def test_tile_windows_by_both_routes_over_the_tallest_plane(G, ns):
    """nbr_win_off(x, y, ns) == nbr_win_off_xy(x | y << 16, ns / 16) == the plain-integer offset, on a plane of ns columns and the
    most rows a context can have (32766): at every tile corner (all four corner pixels of every 16 x 14 tile) and at 10^5 random
    points.  The 12-byte windows of one tile stay inside its 64 bytes, tiles do not overlap, and the furthest window ends inside
    nbr_plane_bytes."""
    sh = SH_MAX
    nt, n_ty = ns // 16, (sh + 13) // 14
    plane = G.geo_plane_bytes(ns, sh)
    assert plane == nt * 64 * n_ty and plane < 2**32

    def offs(x, y):
        x = np.ascontiguousarray(x, np.int32)
        y = np.ascontiguousarray(y, np.int32)
        a = np.zeros(len(x), np.uint32)
        b = np.zeros(len(x), np.uint32)
        G.geo_win_offs(len(x), P(x), P(y), ns, P(a), P(b))
        xl, yl = x.astype(np.int64), y.astype(np.int64)
        want = ((yl // 14) * nt + xl // 16) * 64 + 4 * (yl % 14)
        assert np.array_equal(a.astype(np.int64), want) and np.array_equal(b.astype(np.int64), want)
        return want

    # tile corners: first / last column and first / last row (inside the plane) of every tile
    tx = np.arange(nt, dtype=np.int64)
    ty = np.arange(n_ty, dtype=np.int64)
    top = offs(np.tile(16 * tx, n_ty), np.repeat(14 * ty, nt))
    assert np.array_equal(top, 64 * np.arange(nt * n_ty))            # distinct 64-byte tiles, tile rows contiguous
    offs(np.tile(16 * tx + 15, n_ty), np.repeat(14 * ty, nt))
    y_last = np.minimum(14 * ty + 13, sh - 1)
    bot = offs(np.tile(16 * tx, n_ty), np.repeat(y_last, nt))
    offs(np.tile(16 * tx + 15, n_ty), np.repeat(y_last, nt))
    assert (bot + 12 <= top + 64).all()                              # the last row's window ends with its tile
    assert int(bot.max()) + 12 <= plane
    rng = np.random.default_rng(ns)
    x, y = rng.integers(0, ns, 100000), rng.integers(0, sh, 100000)
    w = offs(x, y)
    tile = (y // 14) * nt + x // 16
    assert ((w >= 64 * tile) & (w + 12 <= 64 * tile + 64)).all() and int(w.max()) + 12 <= plane
    # the two extreme pixels through the scalar exports, in Python integers
    assert G.geo_tile_off(nt - 1, n_ty - 1, ns) == ((n_ty - 1) * nt + nt - 1) * 64 == plane - 64


def test_start_word_leaves_bit_31_to_the_hole_flag():
    """binarise.hip stages a border start as (y * ns + x) | hole << 31 and unpacks pos = e & 0x7fffffff, hole = e >> 31: the largest
    position of the largest plane, row 32765 of 32768 columns, stays below 2^31 (and its int product does not overflow)."""
    y, x = SH_MAX - 1, NS_MAX - 1
    pos = y * NS_MAX + x
    assert pos == SH_MAX * NS_MAX - 1 < 2**30 < 2**31
    for hole in (0, 1):
        e = pos | (hole << 31)
        assert e < 2**32 and (e & 0x7fffffff, e >> 31) == (pos, hole)


def test_frames_the_frame_kernel_cannot_address_are_told_apart(G):
    """hd.h::frame_src_addressable, the rule api.hip refuses frames by: the furthest byte march_unit reads, byte bpp * sw - 1 of row
    sh - 1, must lie inside its 2^31 - 1 byte resource.  Both sides of the bound for every format's bytes per pixel, odd and
    even sizes (the odd last row and column do not count), strides up to INT_MAX, and the frame sizes the header names."""
    assert G.geo_march_src_bytes() == INT_MAX

    def rule(w, h, rs, bpp):
        return ((h & ~1) - 1) * rs + bpp * (w & ~1) <= INT_MAX

    for bpp in (1, 3, 4):
        for (w, h) in ((320, 240), (321, 241), (16, 16), (17, 17), (MAX_SIDE, 600), (600, MAX_SIDE), (16, MAX_SIDE), (MAX_SIDE, 16)):
            sw, sh = w & ~1, h & ~1
            edge = (INT_MAX - bpp * sw) // (sh - 1)       # the largest row_stride the rule accepts
            assert edge >= bpp * w
            for rs in (bpp * w, edge - 1, edge, min(edge + 1, INT_MAX), min(2 * edge, INT_MAX), INT_MAX - 1, INT_MAX):
                want = rule(w, h, rs, bpp)
                assert want == (rs <= edge)
                assert G.geo_frame_src_addressable(w, h, rs, bpp) == int(want), (w, h, rs, bpp)
            assert (sh - 1) * edge + bpp * sw <= INT_MAX < (sh - 1) * (edge + 1) + bpp * sw
    # the bound to the byte: spans of exactly 2^31 - 1 bytes are accepted, of 2^31 refused (16 rows: 15 strides)
    hit = {INT_MAX: 0, INT_MAX + 1: 0}
    for bpp in (1, 3, 4):
        for sw in range(16, 400, 2):
            for span, want in ((INT_MAX, 1), (INT_MAX + 1, 0)):
                if (span - bpp * sw) % 15 == 0:
                    rs = (span - bpp * sw) // 15
                    assert 15 * rs + bpp * sw == span and rs <= INT_MAX
                    assert G.geo_frame_src_addressable(sw, 16, rs, bpp) == want == G.geo_frame_src_addressable(sw + 1, 17, rs, bpp)
                    hit[span] += 1
    assert min(hit.values()) >= 20
    # row 239 of a 320 x 240 frame beyond 2^32: the product must not be formed in 32 bits
    rs = 2**32 // 239 + 1
    assert rs <= INT_MAX and not G.geo_frame_src_addressable(320, 240, rs, 3)
    assert (239 * rs) & 0xffffffff < 2**20   # (wrapped to 32 bits it would look like a tiny, legal span)
    # dense frames: BGR up to 26754 x 26754, four channels up to 23170 x 23170, grey at every size a context can have
    for bpp, ok, bad in ((3, 26754, 26756), (4, 23170, 23172), (1, MAX_SIDE, None)):
        assert G.geo_frame_src_addressable(ok, ok, bpp * ok, bpp) == 1
        if bad:
            assert G.geo_frame_src_addressable(bad, bad, bpp * bad, bpp) == 0


@pytest.mark.parametrize("tall", [False, True], ids=["32767x600", "600x32767"])
def test_what_the_oracle_and_the_host_cores_find_in_the_long_frames(emul, tall):
    """The 32767 x 600 and 600 x 32767 scenes of tests/test_gpu_geometry_limits.py seen by the oracle: markers of all three pasted
    scenes, three or more with every corner beyond 32000, decoded candidates in the strip the far edge cuts -- what that file's
    assertions about the scenes rest on.  And the host builds of the device cores at those coordinates: the square finder
    returns the oracle's squares, the pose core its poses (to the 1e-6 host-to-host bar) under the camera of focal length
    max(w, h)."""
    import geometry_scenes as GS
    from test_device_cores_cpu import emul_squares
    frame, regions = GS.long_frame(tall)
    h, w = frame.shape[:2]
    tpls, cam = H.oracle_templates(GS.LIBRARY), GS.pinhole_camera(w, h)
    markers, cands, grey = H.oracle_registration(frame, tpls, cam)
    axis = 1 if tall else 0
    far = [m for m in markers if (np.array(m.square).reshape(4, 2)[:, axis] >= 32000).all()]
    assert len(markers) >= 6 and len(far) >= 3 and len(cands) >= 100
    for name in ("origin", "centre", "far"):
        assert any(GS.inside(m.square, regions[name]) for m in markers), name
    assert sum(1 for c in cands if c.orient and GS.inside(c.square, regions["cut"])) >= 2
    gray = np.ascontiguousarray(grey[..., 0])
    quads = H.oracle_find_squares(gray)
    assert (quads[:, :, axis].min(axis=1) >= 32000).sum() >= 8
    got = emul_squares(emul, gray)
    assert got.shape == quads.shape and np.array_equal(got, quads)
    for m in markers:
        sq = np.array(m.square, np.float32)
        g = np.zeros(16)
        emul.emul_square_to_glmatrix(P(sq), C.byref(cam), C.c_double(m.aspectRatio), P(g))
        ref = np.array(m.glMatrix)
        assert np.abs(g - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), (np.abs(g - ref).max(), sq.tolist())


def test_the_small_frames_of_the_row_span_tests_have_their_markers_in_the_bottom_rows():
    import geometry_scenes as GS
    frame, truth = GS.bottom_rows_frame(1)
    assert len(truth) == 3 and all(t[:, 1].min() >= 140 for t in truth)
    assert (frame[:140] == GS.CANVAS).all()
    markers, cands, _ = H.oracle_registration(frame, H.oracle_templates(), H.oracle_camera(320, 240))
    assert len(markers) >= 2 and len(cands) >= 9

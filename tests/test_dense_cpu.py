"""CPU tests of dense contexts (ocvar_hip_create_dense): the sparse tracking replay and the chunked square order of the dense
per-frame tail (opencv-ar_amd/csrc/tail_core.h, built for the host from tests/emul/dense_emul.cpp) against the literal loops
they replace, and the new entry points' argument checks, which run before any device call."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import helpers as H
from helpers import P
from hostbuild import host_core


@pytest.fixture(scope="module")
def lib():
    L = host_core("dense_emul")
    L.dense_track_literal.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.dense_track_sparse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p]
    L.dense_order_rank.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.dense_order_sorted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.dense_track_exhaustive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.dense_track_exhaustive.restype = C.c_longlong
    return L


def both(L, marker_squares, squares, w, h):
    """(reserve, n_squares, compacted squares, updated marker squares) of the literal loop and of the sparse replay"""
    out = []
    nm, n = len(marker_squares), len(squares)
    for sparse in (False, True):
        m = (H.Marker * max(nm, 1))()
        for i, s in enumerate(marker_squares):
            m[i].square[:] = [float(v) for v in s]
            m[i].markerId = i
        sq = np.ascontiguousarray(np.asarray(squares, np.float32).reshape(-1, 8)) if n else np.zeros((1, 8), np.float32)
        res = np.full(max(nm * n, 1), -7, np.int32)
        nr = C.c_int(0)
        if sparse:
            dst = np.zeros_like(sq)
            left = L.dense_track_sparse(m, nm, P(sq), n, w, h, P(dst), P(res), len(res), C.byref(nr))
            assert left >= 0
            lst = dst[:left]
        else:
            left = L.dense_track_literal(m, nm, P(sq), n, P(res), len(res), C.byref(nr))
            lst = sq[:left]
        out.append((res[:nr.value].tolist(), left, lst.copy(), np.array([list(m[i].square) for i in range(nm)], np.float32)))
    return out


def assert_same(a, b):
    assert a[0] == b[0]
    assert a[1] == b[1]
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


def square_at(x, y, side=30.0, shift=0):
    c = [(x, y), (x + side, y), (x + side, y + side), (x, y + side)]
    c = c[shift:] + c[:shift]
    return [v for p in c for v in p]


def test_sparse_replay_equals_literal_loop_exhaustive_small(lib):
    """Every list of 0..4 markers x 0..6 squares (with repetition) over small pools around one position: squares on and just
    inside / outside the 20 px boundary, in different cyclic shifts, one within reach only after the marker has moved (15 px
    steps), and equal squares back to back (a match directly followed by a square that would match too: the skip)."""
    b = (100.0, 100.0)
    squares = [square_at(b[0], b[1]), square_at(b[0] + 15, b[1], shift=1), square_at(b[0] + 30, b[1], shift=3),
               square_at(b[0] + 19.99, b[1] - 0.5, shift=2), square_at(b[0] + 20.0, b[1])]
    marks = [square_at(b[0], b[1]), square_at(b[0] + 5, b[1] + 5, shift=2)]
    pool_s = np.ascontiguousarray(np.array(squares, np.float32))
    pool_m = np.ascontiguousarray(np.array(marks, np.float32))
    cases = C.c_longlong(0)
    bad = lib.dense_track_exhaustive(P(pool_m), len(marks), 4, P(pool_s), len(squares), 6, 320, 240, C.byref(cases))
    assert cases.value == sum(2 ** m for m in range(5)) * sum(5 ** n for n in range(7))
    assert bad == 0
    # the skip, spelled out: marker 0 matches squares 0 and 1 equally; the literal loop takes 0 and skips 1
    ms = [square_at(100, 100)]
    sq = [square_at(101, 100), square_at(102, 100), square_at(300, 200), square_at(103, 100)]
    a, c = both(lib, ms, sq, 640, 480)
    assert_same(a, c)
    assert a[0] == [0, 0] and a[1] == 2   # squares 0 and 3 taken, 1 skipped, 2 out of reach
    # updated corners: the marker walks along a row of squares 15 px apart, one step per match
    ms = [square_at(100, 100)]
    sq = [square_at(100 + 15 * k, 100) for k in (1, 0, 2, 4, 3, 5)]
    a, c = both(lib, ms, sq, 640, 480)
    assert_same(a, c)


@pytest.mark.parametrize("nm,n,w,h", [(64, 256, 640, 480), (300, 1800, 1920, 1080), (1300, 5000, 3840, 2160),
                                      (4096, 16384, 3840, 2160)])
def test_sparse_replay_equals_literal_loop_random_frames(lib, nm, n, w, h):
    """random frames up to 4096 markers x 16384 squares: squares on a jittered grid with repeats and strays (some off the frame),
    markers near some of them in random cyclic order"""
    rng = np.random.default_rng(nm + n)
    centres = rng.uniform([-30, -30], [w + 30, h + 30], (max(n // 3, 1), 2))
    sq = []
    for k in range(n):
        cx, cy = centres[rng.integers(0, len(centres))] + rng.normal(0, 6, 2)
        side = rng.uniform(20, 60)
        sq.append(square_at(float(np.float32(cx)), float(np.float32(cy)), float(np.float32(side)), int(rng.integers(0, 4))))
    ms = []
    for k in range(nm):
        s = np.array(sq[rng.integers(0, n)], np.float64).reshape(4, 2) + rng.normal(0, 8, (4, 2))
        s = np.roll(s, int(rng.integers(0, 4)), axis=0)
        ms.append(s.reshape(-1).tolist())
    a, b = both(lib, ms, sq, w, h)
    assert_same(a, b)
    assert len(a[0]) > 0 and a[1] < n   # (the case does exercise matches)


def test_sparse_replay_ignores_non_finite_marker_corners(lib):
    ms = [[float("nan")] * 8, [float("inf")] * 8, square_at(100, 100)]
    sq = [square_at(100, 100), square_at(1e30, -1e30)]
    a, b = both(lib, ms, sq, 640, 480)
    assert_same(a, b)


@pytest.mark.parametrize("n,chunk", [(0, 2048), (1, 2048), (2, 2), (7, 8), (200, 256), (2047, 2048), (2048, 2048), (2049, 2048),
                                     (5000, 2048), (16384, 2048), (1000, 64)])
def test_chunked_order_equals_rank_rule(lib, n, chunk):
    rng = np.random.default_rng(n)
    starts = np.ascontiguousarray(rng.choice(3840 * 2160, size=n, replace=False).astype(np.int32)) if n else np.zeros(1, np.int32)
    a = np.zeros(max(n, 1), np.int32)
    b = np.full(max(n, 1), -1, np.int32)
    lib.dense_order_rank(P(starts), n, P(a))
    lib.dense_order_sorted(P(starts), n, chunk, P(b))
    assert np.array_equal(a[:n], b[:n])
    if n:
        assert sorted(a[:n].tolist()) == list(range(n))   # a permutation: last discovered first


def test_chunked_order_equals_rank_rule_with_repeated_starts(lib):
    """the rank rule sends equal starts to the same slot; the chunked count does the same"""
    rng = np.random.default_rng(5)
    starts = np.ascontiguousarray(rng.integers(0, 3000, 6000).astype(np.int32))
    a = np.zeros(6000, np.int32)
    b = np.zeros(6000, np.int32)
    lib.dense_order_rank(P(starts), 6000, P(a))
    lib.dense_order_sorted(P(starts), 6000, 2048, P(b))
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    import opencv_ar_amd
    return opencv_ar_amd


def test_dense_entry_points_declared_and_exported(pkg):
    header = open(os.path.join(H.ROOT, "include", "ocvar_hip.h")).read()
    for name in ("ocvar_hip_create_dense", "ocvar_hip_max_markers"):
        assert name + "(" in header and name in pkg.HIP_SYMBOLS
        assert hasattr(pkg.hip_lib(), name)
    assert "OCVAR_MAX_QUADS_DENSE = 16384" in header and "OCVAR_MAX_MARKERS_DENSE = 4096" in header


@pytest.mark.parametrize("q,m", [(0, 64), (16385, 64), (256, 0), (256, 4097), (-1, -1)])
def test_create_dense_rejects_out_of_range_limits(pkg, q, m):
    """OCVAR_E_ARG (-2) for squares outside 1..16384 or markers outside 1..4096, decided before any device call (no GPU here)"""
    lib = pkg.hip_lib()
    ctx = C.c_void_p()
    assert lib.ocvar_hip_create_dense(C.byref(ctx), 0, 1920, 1080, 1, q, m) == -2
    assert not ctx
    assert lib.ocvar_hip_max_markers(None) == -2
    with pytest.raises(pkg.OcvarError):
        pkg.Detector(1920, 1080, 1, max_quads=q, max_markers=m)


def test_detectors_made_without_init_keep_the_default_stride(pkg):
    det = pkg.Detector.__new__(pkg.Detector)
    assert det.max_markers == pkg.MAX_MARKERS == 64 and det.max_quads == pkg.MAX_QUADS
    pm, pc = det._prev_arrays([list(np.zeros(3, pkg.MARKER_DTYPE))], 1)
    assert pm.shape == (1, 64) and pc.tolist() == [3]


# ---- the frame builders of tests/test_gpu_dense_limits.py hit their exact oracle counts ----

LIMIT_QS = [1, 63, 64, 65, 255, 256, 2047, 2048, 2049, 4097, 16384]
LIMIT_MS = [1, 7, 64, 65]


def test_squares_frame_hits_every_exact_count_of_the_limit_tests():
    import dense_synth as D
    for n in sorted({n for q in LIMIT_QS for n in (q - 1, q, q + 1)}):
        g = D.squares_frame(n)   # (asserts the oracle's count itself)
        assert len(D.oracle_squares(g)) == n and g.shape[::-1] == D.frame_size_for(n)
    for w, h in ((3839, 2157), (1001, 999)):   # (frame sides that are not multiples of 32, squares up to 4 px from the border)
        n = len(D.square_slots(w, h, margin=4))
        assert len(D.oracle_squares(D.squares_frame(n, w, h, margin=4))) == n
    with pytest.raises(AssertionError):
        D.squares_frame(len(D.square_slots(640, 480)) + 1, 640, 480)


def test_squares_frame_around_a_marker_strip():
    import dense_synth as D
    names = D.library(3)
    strip = D.marker_strip(1, names)
    have = D.strip_squares(strip, 3840, 2160)
    assert have >= 1
    for n in (have + 4095, have + 4096):
        g = D.squares_frame(n, 3840, 2160, marker_strip=strip)
        assert len(D.oracle_squares(g)) == n and np.array_equal(g[:100, :100], strip)
    tpls, cam = H.oracle_templates(names), H.oracle_camera(3840, 2160)
    m, _, _ = H.oracle_registration(np.repeat(g[:, :, None], 3, axis=2), tpls, cam, max_markers=20000, max_cands=100000)
    assert len(m) == 1 and m[0].templateId == 0   # (the strip's marker decodes; the solid squares give no candidate)


def test_marker_frame_hits_every_exact_marker_count():
    import dense_synth as D
    names = D.library(66, seed=11)
    tpls, cam = H.oracle_templates(names), H.oracle_camera(1920, 1080)
    for k in sorted({k for m in LIMIT_MS for k in (m - 1, m, m + 1)}):
        m, _, _ = H.oracle_registration(D.marker_frame(k, names), tpls, cam, max_markers=20000, max_cands=100000)
        assert len(m) == k, (k, len(m))
        assert sorted(r.templateId for r in m) == list(range(k))


def test_concentric_frame_squares_nest():
    import dense_synth as D
    g = D.concentric_frame(3840, 2160)
    sq = D.oracle_squares(g)
    targets = len(range(20, 2160 - 120 - 20, 150)) * len(range(20, 3840 - 120 - 20, 150))
    assert len(sq) >= 3 * targets


def test_oracle_registration_sees_more_than_4096_squares():
    """the reference's square list is unbounded: a frame past the oracle's first buffer is not a frame without squares"""
    import dense_synth as D
    g = D.squares_frame(4097)
    sq = D.oracle_squares(g)
    prev = (H.Marker * 1)()
    prev[0].square[:] = [float(v) for v in sq[-1].reshape(-1)]
    prev[0].aspectRatio = 1.0
    h, w = g.shape
    m, _, _ = H.oracle_registration(np.repeat(g[:, :, None], 3, axis=2), H.oracle_templates(), H.oracle_camera(w, h),
                                    prev=list(prev), max_markers=16, max_cands=16)
    assert len(m) >= 1 and list(m[0].square) == [float(v) for v in sq[-1].reshape(-1)]   # (tracked: the first record)

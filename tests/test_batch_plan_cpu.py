"""CPU tests of the workspace sizing and the batch plan (opencv-ar_amd/csrc/plan_core.h, built for the host from
tests/emul/plan_emul.cpp): the numbers api.hip allocates and launches by, and the kernels rely on -- binarise.hip on work units
of whole tile rows that cover the plane, the followers on grids within their slabs."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from hostbuild import host_core

KNOBS = ("crop_phases", "mid_steps", "mid_blocks", "long_blocks", "short_blocks", "min_units")   # PlanOverrides' order
SIDES = (16, 17, 239, 240, 241, 255, 256, 257, 32767)
MAX_QUADS, MAX_MARKERS = 256, 64                  # ocvar_hip_create
DENSE_QUADS, DENSE_MARKERS = 16384, 4096          # the limits of ocvar_hip_create_dense


class PlanOut(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("cap_pool_ints", "cap_crop_pixels")] + [(n, C.c_int) for n in (
        "cap_frame_cands", "cap_crop_cands", "cap_crop_rois", "cap_crop_tiles", "cap_crop_quads", "cap_long",
        "max_mid_blocks", "max_long_blocks", "track_gw", "track_gh", "decode_slices", "order_chunk",
        "W", "H", "sw", "sh", "ns", "n_frames",
        "frame_strips", "frame_chunk_rows", "frame_chunks", "mid_steps", "crop_phases", "mid_blocks", "long_blocks",
        "short_blocks", "crop_blocks")]


@pytest.fixture(scope="module")
def lib():
    L = host_core("plan_emul")
    L.plan_emul.argtypes = [C.c_int] * 10 + [C.c_void_p, C.c_void_p, C.POINTER(PlanOut)]
    L.plan_emul.restype = None
    assert L.plan_emul_march_strip() == 240 and L.plan_emul_tile_rows() == 14
    return L


def plan(lib, w, h, n_frames, max_batch=None, gated=False, dense=False, max_w=None, max_h=None, max_quads=None,
         max_markers=None, **knobs):
    """the plan of a batch of n_frames w x h frames on a context made for max_batch (default: n_frames) frames of max_w x max_h
    (default: w x h); knobs: overrides by PlanOverrides' names"""
    assert set(knobs) <= set(KNOBS)
    ks = np.array([k in knobs for k in KNOBS], dtype=np.int32)
    kv = np.array([knobs.get(k, 0) for k in KNOBS], dtype=np.int64)
    o = PlanOut()
    lib.plan_emul(max_w or w, max_h or h, max_batch or n_frames, max_quads or (DENSE_QUADS if dense else MAX_QUADS),
                  max_markers or (DENSE_MARKERS if dense else MAX_MARKERS), int(dense), w, h, n_frames, int(gated),
                  H.P(ks) if knobs else None, H.P(kv) if knobs else None, C.byref(o))
    return o


def check_invariants(o, w, h, n_frames):
    where = (w, h, n_frames)
    assert (o.W, o.H, o.n_frames) == where
    assert o.sw == w & ~1 and o.sh == h & ~1
    assert o.frame_chunk_rows % 14 == 0 and o.frame_chunk_rows >= 14, where
    assert o.frame_chunks * o.frame_chunk_rows >= o.sh > (o.frame_chunks - 1) * o.frame_chunk_rows, where
    assert o.frame_strips * 240 >= o.sw > (o.frame_strips - 1) * 240, where
    assert o.ns % 16 == 0 and o.ns >= o.sw, where
    assert 1 <= o.mid_blocks <= o.max_mid_blocks <= 1024, where
    assert 1 <= o.long_blocks <= o.max_long_blocks <= 1024, where
    assert 1 <= o.short_blocks <= 65535, where
    assert 1 <= o.crop_blocks <= 65535, where
    assert o.mid_steps >= 32, where
    assert o.crop_phases in (1, 2), where
    assert 0 < o.cap_frame_cands <= 1 << 30 and o.cap_crop_cands == o.cap_frame_cands, where
    assert 0 < o.cap_crop_tiles <= 1 << 30, where
    assert 0 < o.cap_long <= 1 << 28, where
    assert o.cap_crop_rois > 0 and o.cap_crop_quads > 0 and o.cap_pool_ints > 0 and o.cap_crop_pixels > 0, where


def test_invariants_over_the_admitted_range(lib):
    """What the kernels rely on holds for every frame size (the sizes around the strip width 240 and the tile width 16, the
    smallest and the largest side, and a seeded sample), every batch size around the thresholds 8 and 128 up to max_batch, with
    and without a gate, on plain and dense contexts of small and large max_batch."""
    rng = np.random.default_rng(20240607)
    sizes = [(w, h) for w in SIDES for h in SIDES] + [tuple(int(v) for v in rng.integers(16, 32768, 2)) for _ in range(60)]
    for max_batch in (1, 9, 2048, 4096):
        frames = sorted({n for n in (1, 8, 9, 127, 128, 2048) if n <= max_batch} | {max_batch})
        for dense in (False, True):
            for gated in (False, True):
                for w, h in sizes:
                    for n in frames:
                        o = plan(lib, w, h, n, max_batch=max_batch, gated=gated, dense=dense)
                        check_invariants(o, w, h, n)
                        if dense:
                            assert o.track_gw * 32 >= w > (o.track_gw - 1) * 32 and o.track_gh * 32 >= h > (o.track_gh - 1) * 32
                            assert 4 <= o.decode_slices <= 64 and o.order_chunk == 2048


def test_invariants_of_a_smaller_batch_on_a_larger_context(lib):
    """frames smaller than the context's limits (the grids' limits come from the context, the geometry from the batch)"""
    for gated in (False, True):
        for w, h in ((16, 16), (241, 17), (640, 480), (1919, 1079)):
            for n in (1, 8, 9, 127, 128, 2048):
                o = plan(lib, w, h, n, max_batch=2048, gated=gated, max_w=1920, max_h=1080)
                check_invariants(o, w, h, n)
                assert (o.max_mid_blocks, o.max_long_blocks, o.cap_frame_cands) == (1024, 1024, 265420800)


def test_capacity_clamps(lib):
    """the clamps the sizing states (1 << 30 start candidates and crop work units, 1 << 28 tier survivors) take hold on huge contexts"""
    o = plan(lib, 32767, 32767, 1, max_batch=300000)
    check_invariants(o, 32767, 32767, 1)
    assert (o.cap_frame_cands, o.cap_crop_tiles, o.cap_long) == (1 << 30, 1 << 30, 1 << 28)
    o = plan(lib, 16, 16, 1, max_batch=65536)   # (the largest max_batch below the clamps)
    assert (o.cap_frame_cands, o.cap_crop_tiles, o.cap_long) == (1 << 30, 65536 * 4096, 1 << 28)
    o = plan(lib, 16, 16, 1, max_batch=65535)
    assert (o.cap_frame_cands, o.cap_long) == (65535 * 16384, 65535 * 4096)


def test_overrides(lib):
    base = dict(max_batch=2048, max_w=1920, max_h=1080)
    for gated in (False, True):
        for n in (1, 2048):
            d = plan(lib, 1920, 1080, n, gated=gated, **base)
            # in range: taken
            assert plan(lib, 1920, 1080, n, gated=gated, crop_phases=1, **base).crop_phases == 1
            assert plan(lib, 1920, 1080, n, gated=gated, crop_phases=2, **base).crop_phases == 2
            for v in (32, 33, 500, 100000):
                assert plan(lib, 1920, 1080, n, gated=gated, mid_steps=v, **base).mid_steps == v
            for v in (1, 7, 1024):
                assert plan(lib, 1920, 1080, n, gated=gated, mid_blocks=v, **base).mid_blocks == v
                assert plan(lib, 1920, 1080, n, gated=gated, long_blocks=v, **base).long_blocks == v
            for v in (1, 1025, 65535):
                assert plan(lib, 1920, 1080, n, gated=gated, short_blocks=v, **base).short_blocks == v
            # out of range: the grids fall back to their maximum (tier 1: 1024), short step budgets become 32, phases 2
            for v in (0, -1, 1025, 1 << 20):
                assert plan(lib, 1920, 1080, n, gated=gated, mid_blocks=v, **base).mid_blocks == 1024
                assert plan(lib, 1920, 1080, n, gated=gated, long_blocks=v, **base).long_blocks == 1024
            for v in (0, -1, 65536, 1 << 20):
                assert plan(lib, 1920, 1080, n, gated=gated, short_blocks=v, **base).short_blocks == 1024
            for v in (31, 1, 0, -5):
                assert plan(lib, 1920, 1080, n, gated=gated, mid_steps=v, **base).mid_steps == 32
            for v in (0, 2, 3, -1, 100):
                assert plan(lib, 1920, 1080, n, gated=gated, crop_phases=v, **base).crop_phases == 2
            # a knob changes its own field only
            o = plan(lib, 1920, 1080, n, gated=gated, mid_blocks=7, **base)
            assert [getattr(o, f) for f, _ in PlanOut._fields_ if f != "mid_blocks"] == \
                   [getattr(d, f) for f, _ in PlanOut._fields_ if f != "mid_blocks"]
    # a context with smaller slabs: the fall-back is that context's maximum
    o = plan(lib, 640, 480, 9, mid_blocks=33, long_blocks=129)
    assert (o.max_mid_blocks, o.mid_blocks, o.max_long_blocks, o.long_blocks) == (32, 32, 128, 128)
    # min_units: the work units below which chunks are not made taller (1080p: 8 strips, at most 8 chunks of 140 rows)
    assert [plan(lib, 1920, 1080, 1, min_units=v).frame_chunks for v in (65536, 33, 32, 16, 8, 1, 0, -1)] == [8, 8, 4, 2, 1, 1, 1, 1]
    assert [plan(lib, 1920, 1080, 1, min_units=v).frame_chunk_rows for v in (33, 32, 16, 8)] == [140, 280, 546, 1092]


# W, H, n_frames = max_batch, gated: strips, chunk_rows, chunks, mid_steps, phases, mid_blocks, long_blocks, short, crop_blocks
BATCH_PINS = [
    ((1920, 1080, 2048, False), (8, 280, 4, 1536, 2, 1024, 1024, 1024, 2048)),
    ((1920, 1080, 2048, True), (8, 1092, 1, 1536, 2, 256, 1024, 1024, 2048)),
    ((1920, 1080, 1, False), (8, 140, 8, 128, 1, 32, 128, 16, 32)),
    ((16, 16, 1, False), (1, 28, 1, 128, 1, 32, 128, 16, 32)),
    ((17, 17, 1, False), (1, 28, 1, 128, 1, 32, 128, 16, 32)),
    ((640, 480, 9, True), (3, 126, 4, 1536, 2, 32, 128, 72, 144)),
    ((32767, 16, 128, False), (137, 28, 1, 1536, 2, 128, 1024, 1024, 2048)),
    ((16, 32767, 1, False), (1, 140, 235, 128, 1, 32, 128, 16, 32)),
]


@pytest.mark.parametrize("case,want", BATCH_PINS, ids=["%dx%d-n%d-%s" % (c[0], c[1], c[2], "gated" if c[3] else "alone") for c, _ in BATCH_PINS])
def test_pinned_batch_plans(lib, case, want):
    w, h, n, gated = case
    o = plan(lib, w, h, n, gated=gated)
    assert (o.frame_strips, o.frame_chunk_rows, o.frame_chunks, o.mid_steps, o.crop_phases, o.mid_blocks, o.long_blocks,
            o.short_blocks, o.crop_blocks) == want
    assert (o.sw, o.sh, o.ns) == (w & ~1, h & ~1, ((w & ~1) + 15) // 16 * 16)


def test_pinned_capacities(lib):
    o = plan(lib, 1920, 1080, 1)
    assert (o.cap_frame_cands, o.cap_long, o.cap_pool_ints, o.cap_crop_pixels) == (129600, 262144, 17039360, 2106368)
    assert (o.cap_crop_rois, o.cap_crop_tiles, o.cap_crop_quads, o.max_mid_blocks, o.max_long_blocks) == (256, 4096, 1024, 32, 128)
    o = plan(lib, 1920, 1080, 2048)
    assert (o.cap_frame_cands, o.cap_long, o.cap_pool_ints, o.cap_crop_pixels) == (265420800, 8388608, 553648128, 4313841664)
    assert (o.cap_crop_rois, o.cap_crop_tiles, o.cap_crop_quads) == (2048 * 256, 2048 * 4096, 2048 * 1024)
    assert plan(lib, 16, 16, 1).cap_frame_cands == 16384


def test_pinned_dense_contexts(lib):
    """dense contexts: four crop work units per square, four times the crop planes, the tracking grid in cells of 32 px, decode
    waves and sort chunks by the squares per frame"""
    o = plan(lib, 1920, 1080, 4, dense=True)   # 16384 squares, 4096 markers per frame
    assert (o.track_gw, o.track_gh, o.decode_slices, o.order_chunk) == (60, 34, 64, 2048)
    assert (o.cap_crop_rois, o.cap_crop_tiles, o.cap_crop_quads, o.cap_crop_pixels) == (65536, 262144, 262144, 33701888)
    assert (o.cap_frame_cands, o.cap_long, o.cap_pool_ints) == (518400, 262144, 17825792)
    o = plan(lib, 640, 480, 1, dense=True, max_quads=100, max_markers=10)
    assert (o.track_gw, o.track_gh, o.decode_slices, o.order_chunk) == (20, 15, 4, 128)
    assert (o.cap_crop_rois, o.cap_crop_tiles, o.cap_crop_quads, o.cap_crop_pixels) == (100, 4096, 400, 1280512)
    o = plan(lib, 33, 16, 1, dense=True, max_quads=1, max_markers=1)
    assert (o.track_gw, o.track_gh, o.decode_slices, o.order_chunk) == (2, 1, 4, 2)
    for q, chunk, slices in ((2, 2, 4), (3, 4, 4), (320, 512, 5), (2048, 2048, 32), (2049, 2048, 32), (4096, 2048, 64)):
        o = plan(lib, 640, 480, 1, dense=True, max_quads=q)
        assert (o.order_chunk, o.decode_slices) == (chunk, slices), q
    # the plain context of the same size: a quarter of the crop planes, no dense fields
    o = plan(lib, 1920, 1080, 4)
    assert (o.cap_crop_pixels, o.cap_crop_tiles, o.track_gw, o.decode_slices, o.order_chunk) == (8425472, 16384, 0, 0, 0)

"""CPU tests of the crop pass's lists and step budget (opencv-ar_amd/csrc/croplist_core.h, built for the host from
tests/emul/croplist_emul.cpp, which walks the lists the way follow.hip::crop_lists does) and of the plan's
crop_steps_cap (plan_core.h).

The rules the lists must restate are those follow_mid_kernel applied at hand-out before the lists existed: phase 1 took an
entry of mid_crop when pos == crop_min_rest[roi]; phase 2 when pos != crop_min_rest[roi] and not
(best_crop[roi] >> 32) < pos (unsigned).  They are written out again below, in numpy."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from hostbuild import host_core

KNOBS = ("crop_phases", "mid_steps", "mid_blocks", "long_blocks", "short_blocks", "min_units")   # PlanOverrides' order
NO_START = 0x7fffffff
NO_QUAD = 0xffffffffffffffff


@pytest.fixture(scope="module")
def lib():
    L = host_core("croplist_emul")
    L.croplist_emul_split.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.croplist_emul_prune.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.croplist_emul_plan.argtypes = [C.c_int] * 5 + [C.c_void_p] * 3
    assert L.croplist_emul_no_start() == NO_START
    return L


def split(lib, src, min_rest, waves):
    n = len(src)
    e, r = np.zeros((n + 1, 3), np.int32), np.zeros((n + 1, 3), np.int32)
    ne, nr = C.c_int(-1), C.c_int(-1)
    lib.croplist_emul_split(H.P(src), n, H.P(min_rest), waves, H.P(e), C.byref(ne), H.P(r), C.byref(nr))
    return e[:ne.value], r[:nr.value]


def prune(lib, src, best, waves):
    n = len(src)
    out = np.zeros((n + 1, 3), np.int32)
    no = C.c_int(-1)
    lib.croplist_emul_prune(H.P(np.ascontiguousarray(src)), n, H.P(best), waves, H.P(out), C.byref(no))
    return out[:no.value]


def rows(a):
    """a list as a sorted multiset of (roi, pos, is_hole)"""
    return sorted(map(tuple, np.asarray(a).reshape(-1, 3).tolist()))


def random_case(rng, n_crops, n_entries, plane=60000):
    """tier 1's output for n_crops crops: mid_crop in arbitrary order, crop_min_rest as its atomicMin leaves it, and a
    best_crop table as phase 1 might leave it"""
    roi = rng.integers(0, n_crops, n_entries).astype(np.int32)
    # (few distinct positions per crop: ties with the earliest start and with the best quad's start do occur)
    pos = rng.integers(1, plane, n_entries).astype(np.int32) if n_entries == 0 or rng.random() < 0.5 else \
        (1 + 97 * rng.integers(0, 12, n_entries)).astype(np.int32)
    src = np.ascontiguousarray(np.stack([roi, pos, rng.integers(0, 2, n_entries).astype(np.int32)], axis=1))
    min_rest = np.full(n_crops, NO_START, np.int32)          # crops tier 1 routed no start of keep 0x7fffffff
    np.minimum.at(min_rest, roi, pos)
    best = np.full(n_crops, NO_QUAD, np.uint64)              # crops without a quad keep ~0
    for c in range(n_crops):
        kind = rng.integers(0, 4)
        if kind == 1:      # the quad of the crop's frame border: starts before every entry
            best[c] = (np.uint64(rng.integers(0, 2)) << np.uint64(32)) | np.uint64(rng.integers(0, 1 << 20))
        elif kind >= 2 and min_rest[c] != NO_START:   # the quad of one of the crop's own starts
            mine = pos[roi == c]
            best[c] = (np.uint64(rng.choice(mine)) << np.uint64(32)) | np.uint64(rng.integers(0, 1 << 20))
    return src, min_rest, best


@pytest.mark.parametrize("n_crops,n_entries,waves", [(1, 0, 1), (1, 1, 1), (3, 63, 1), (5, 64, 2), (40, 511, 1), (40, 512, 3),
                                                      (64, 513, 2), (300, 2500, 4), (700, 6000, 3), (700, 6000, 16), (9, 4000, 5)])
def test_lists_hold_exactly_what_the_old_hand_out_rules_took(lib, n_crops, n_entries, waves):
    rng = np.random.default_rng(1000 * n_crops + n_entries + waves)
    for rep in range(4):
        src, min_rest, best = random_case(rng, n_crops + rep, n_entries)   # (crops beyond the routed ones: never indexed, stay NO_START)
        e, r = split(lib, src, min_rest, waves)
        assert rows(np.concatenate([e, r])) == rows(src)                   # E u R is the input, nothing twice
        earliest = src[:, 1] == min_rest[src[:, 0]]
        assert rows(e) == rows(src[earliest])                              # phase 1's old rule
        live = prune(lib, r, best, waves)
        beaten = (best[src[:, 0]] >> np.uint64(32)).astype(np.uint32) < src[:, 1].astype(np.uint32)
        assert rows(live) == rows(src[~earliest & ~beaten])                # phase 2's old rule
        if n_entries:
            routed = np.unique(src[:, 0])
            assert (min_rest[routed] != NO_START).all() and len(e) >= len(routed)   # every routed crop has its earliest start in E


def test_crops_without_a_routed_start_and_without_a_quad(lib):
    # crop 0: routed starts, no quad -> everything but the earliest stays live; crop 1: no routed start at all; crop 2: a quad
    # whose start precedes every entry -> nothing stays live; crop 3: a quad at its second start -> that start and the ones
    # before it stay (a start equal to the best one is not behind it)
    src = np.array([[0, 50, 0], [0, 40, 1], [0, 60, 0], [2, 500, 0], [2, 300, 1], [3, 10, 0], [3, 20, 0], [3, 30, 1], [3, 15, 0]], np.int32)
    min_rest = np.array([40, NO_START, 300, 10], np.int32)
    best = np.array([NO_QUAD, NO_QUAD, (17 << 32) | 5, (20 << 32) | 9], np.uint64)
    e, r = split(lib, src, min_rest, 1)
    assert rows(e) == [(0, 40, 1), (2, 300, 1), (3, 10, 0)]
    assert rows(r) == [(0, 50, 0), (0, 60, 0), (2, 500, 0), (3, 15, 0), (3, 20, 0), (3, 30, 1)]
    assert rows(prune(lib, r, best, 1)) == [(0, 50, 0), (0, 60, 0), (3, 15, 0), (3, 20, 0)]


def plan(lib, w, h, n_frames, max_batch=None, gated=False, **knobs):
    ks = np.array([k in knobs for k in KNOBS], dtype=np.int32)
    kv = np.array([knobs.get(k, 0) for k in KNOBS], dtype=np.int64)
    out = np.zeros(3, np.int32)
    lib.croplist_emul_plan(w, h, n_frames, max_batch or n_frames, int(gated), H.P(ks) if knobs else None, H.P(kv) if knobs else None,
                           H.P(out))
    return dict(mid_steps=int(out[0]), crop_steps_cap=int(out[1]), crop_phases=int(out[2]))


def test_crop_steps_cap_of_the_plan(lib):
    for (w, h) in ((1920, 1080), (640, 480), (16, 16)):
        for gated in (False, True):
            for n in (1, 2, 8):                          # latency plans: the short budget on purpose
                p = plan(lib, w, h, n, max_batch=64, gated=gated)
                assert p["mid_steps"] == 128 and p["crop_steps_cap"] == 128, (w, h, n)
            for n in (9, 16, 64, 2048):                  # throughput plans
                p = plan(lib, w, h, n, gated=gated)
                assert p["mid_steps"] == 1536 and p["crop_steps_cap"] == 3072, (w, h, n)
            for n in (1, 8, 9, 2048):                    # every mid_steps override: the caller's budget holds for crops too
                for ms in (1, 32, 64, 128, 1536, 1537, 3072, 5000):
                    p = plan(lib, w, h, n, gated=gated, mid_steps=ms)
                    assert p["mid_steps"] == max(ms, 32) and p["crop_steps_cap"] == p["mid_steps"], (w, h, n, ms)
            # the other knobs leave it alone
            p = plan(lib, w, h, 9, gated=gated, crop_phases=1, mid_blocks=3, long_blocks=2, short_blocks=5, min_units=1)
            assert p["crop_steps_cap"] == 3072 and p["crop_phases"] == 1
            p = plan(lib, w, h, 8, gated=gated, crop_phases=2)
            assert p["crop_steps_cap"] == 128 and p["crop_phases"] == 2


def test_walk_budget_fits_the_crop(lib):
    b = lib.croplist_emul_budget
    assert b(250, 250, 1536, 3072) == 3008               # 6 x 500 rounded up to whole blocks of 32 steps
    assert b(128, 128, 1536, 3072) == 1536               # 6 x 256 = 1536 exactly
    assert b(128, 130, 1536, 3072) == 1568
    assert b(20, 20, 1536, 3072) == 1536                 # never below the batch's mid_steps
    assert b(260, 260, 1536, 3072) == 3072               # never above the cap
    assert b(32766, 32766, 1536, 3072) == 3072
    for cap in (32, 64, 128, 1536, 5000):                # cap == mid_steps: the budget is mid_steps whatever the crop
        for side in (2, 64, 250, 4000):
            assert b(side, side, cap, cap) == cap
    last = 0
    for s in range(2, 600, 2):
        v = b(s, s + 2, 1536, 3072)
        assert 1536 <= v <= 3072 and v % 32 == 0 and v >= last
        assert v == 3072 or v == 1536 or 0 <= v - 6 * (2 * s + 2) < 32
        last = v

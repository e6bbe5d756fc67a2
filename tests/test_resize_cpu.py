"""The resize core (opencv-ar_amd/csrc/resize_core.h) on the host (tests/resize_chain.py builds it) against an independent numpy
restatement of the rules, byte for byte; what the rules promise (copies, constants, the exact factor 2, integer boxes, table
weights); the record map against numpy float64; the chain "shrink by 2, detect, map the squares back up" through the oracle; and
the stand-alone program under the sanitizers.  tests/test_gpu_resize.py holds the kernels to this build byte for byte."""

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import persp_synth as PS
import resize_chain as RC
from helpers import P
from hostbuild import run_sanitized

SIDES = [1, 2, 3, 5, 8, 17, 64]
PAIRS = [(64, 32), (96, 32), (48, 32), (33, 7), (7, 33), (1, 9)]
CHANNELS = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "gray": 1}


@pytest.fixture(scope="module")
def L():
    return RC.build_emul()


def sweep_sizes():
    """(sw, sh, dw, dh): every (source, destination) width pair of SIDES with a height pair drawn from the same list by a fixed
    permutation, then the fixed pairs along either axis and along both"""
    wp = [(s, d) for s in SIDES for d in SIDES]
    out = [(sw, wp[(5 * j + 3) % len(wp)][0], dw, wp[(5 * j + 3) % len(wp)][1]) for j, (sw, dw) in enumerate(wp)]
    for s, d in PAIRS:
        out += [(s, 5, d, 3), (5, s, 5, d), (s, s, d, d)]
    # and every width pair AREA takes with a height pair it takes: the permutation's, larger side first, or an equal pair
    for sw, sh, dw, dh in list(out):
        if dw <= sw <= RC.MAX_RATIO * dw and not RC.area_ok(sw, sh, dw, dh):
            hi, lo = max(sh, dh), min(sh, dh)
            out.append((sw, hi, dw, lo if hi <= RC.MAX_RATIO * lo else hi))
    return out


@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("interp", list(RC.INTERPS))
def test_case_sweep(L, interp, fmt):
    """guarded frames with padded rows: the numpy restatement's pixels, every guard byte kept; AREA beyond its domain is refused
    with nothing written"""
    ch = CHANNELS[fmt]
    done = refused = 0
    kinds = set()
    for j, (sw, sh, dw, dh) in enumerate(sweep_sizes()):
        n = 1 + j % 2
        src = FK.pix_layout(n, sw, sh, fmt, aligned=bool(j & 2), seed=j)
        dst = FK.pix_layout(n, dw, dh, fmt, aligned=bool(j & 4), fill=FK.GUARD)
        rc, out = RC.host_resize(L, src, dst, interp)
        if interp == "area" and not RC.area_ok(sw, sh, dw, dh):
            assert rc == FK.E_ARG and (out == FK.GUARD).all(), (sw, sh, dw, dh)
            refused += 1
            continue
        assert rc == 0
        assert (out[~dst.pixel_mask()] == FK.GUARD).all(), (sw, sh, dw, dh)
        plan = np.zeros(3, np.int32)
        L.resize_plan_emul(sw, sh, dw, dh, RC.INTERPS[interp], P(plan))
        assert tuple(plan) == RC.np_plan(sw, sh, dw, dh, interp), (sw, sh, dw, dh)
        kinds.add(int(plan[0]))
        for f in range(n):
            want = RC.np_resize(src.view(f), dw, dh, interp)
            got = dst.view(f, out)
            assert got.shape == (dh, dw, ch)
            assert np.array_equal(got, want), (interp, fmt, sw, sh, dw, dh, f, np.argwhere(got != want)[:3].tolist())
        done += 1
    assert done >= 30 and (refused >= 10) == (interp == "area")
    assert kinds == {"nearest": {0}, "linear": {1, 2}, "area": {2, 3}}[interp]


# ---- LINEAR ---------------------------------------------------------------------------------------------------------------------------

RATIO_SIZES = [(s, d) for s in (1, 2, 3, 5, 7, 8, 17, 33, 64, 100) for d in (1, 2, 3, 5, 7, 8, 9, 17, 33, 64, 100)]


def test_linear_of_equal_sizes_is_a_copy(L):
    rng = np.random.default_rng(1)
    for w, h, ch in [(1, 1, 1), (5, 3, 3), (64, 17, 4), (33, 8, 1)]:
        img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        assert np.array_equal(RC.host_resize_image(L, img, w, h, "linear"), img)
        assert np.array_equal(RC.host_resize_image(L, img, w, h, "nearest"), img)
        assert np.array_equal(RC.host_resize_image(L, img, w, h, "area"), img)


def test_linear_keeps_a_constant_image_constant(L):
    """the two weights of an axis are rounded on their own and need not sum to 2048: the result must not show it"""
    off = 0
    for s, d in RATIO_SIZES:
        t = np.zeros(4, np.int32)
        for x in range(d):
            L.resize_linear_tap_emul(x, s, d, P(t))
            off += int(t[2] + t[3] != 2048)
        for v in (0, 1, 127, 128, 254, 255):
            img = np.full((s, s, 1), v, np.uint8)
            out = RC.host_resize_image(L, img, d, (d * 3 + 1) // 2, "linear")
            assert (out == v).all(), (s, d, v, np.unique(out).tolist())
    print("LINEAR: %d destination indices whose weights do not sum to 2048" % off)


def test_linear_by_exactly_two_is_area(L):
    rng = np.random.default_rng(2)
    for w, h, ch in [(1, 1, 3), (7, 5, 1), (32, 9, 4)]:
        img = rng.integers(0, 256, (2 * h, 2 * w, ch), dtype=np.uint8)
        lin, area = RC.host_resize_image(L, img, w, h, "linear"), RC.host_resize_image(L, img, w, h, "area")
        assert np.array_equal(lin, area)
        assert np.array_equal(area, ((img.astype(np.int64).reshape(h, 2, w, 2, ch).sum((1, 3)) + 2) >> 2).astype(np.uint8))
        # a factor of two along one axis only stays linear
        one = RC.host_resize_image(L, img, w, 2 * h, "linear")
        assert np.array_equal(one, RC.np_resize(img, w, 2 * h, "linear"))
    plan = np.zeros(3, np.int32)
    L.resize_plan_emul(64, 48, 32, 24, 1, P(plan))
    assert tuple(plan) == (RC.KIND_BOX, 2, 2)
    L.resize_plan_emul(64, 48, 32, 48, 1, P(plan))
    assert plan[0] == RC.KIND_LINEAR


# ---- AREA -----------------------------------------------------------------------------------------------------------------------------

def test_area_keeps_a_constant_image_constant(L):
    for s, d in RATIO_SIZES:
        if d > s or s > RC.MAX_RATIO * d:
            continue
        for v in (0, 1, 127, 128, 254, 255):
            img = np.full((s, s, 1), v, np.uint8)
            out = RC.host_resize_image(L, img, d, d, "area")
            assert (out == v).all(), (s, d, v, np.unique(out).tolist())
            out = RC.host_resize_image(L, img, d, s, "area")   # (one axis kept: the table on a whole-number axis)
            assert (out == v).all(), (s, d, v)


@pytest.mark.parametrize("k", [2, 3, 4, 16])
def test_area_integer_box_is_the_rounded_mean(L, k):
    """int64 sums; 2 x 2 rounds halves up by its shift, every other block rounds the float32 product to nearest even"""
    rng = np.random.default_rng(k)
    for w, h, ch in [(1, 1, 1), (5, 3, 3), (9, 2, 4)]:
        img = rng.integers(0, 256, (k * h, k * w, ch), dtype=np.uint8)
        img[:k, :k] = 255     # the largest sum
        total = img.astype(np.int64).reshape(h, k, w, k, ch).sum((1, 3))
        if k == 2:
            want = (total + 2) >> 2
        else:
            want = np.clip(np.rint(total.astype(np.float32) * np.float32(1.0 / (k * k))), 0, 255)
            assert np.abs(want - total / (k * k)).max() <= 0.5 + 1e-3   # (and that is the mean, rounded)
        assert np.array_equal(RC.host_resize_image(L, img, w, h, "area"), want.astype(np.uint8))
    # a block that is not square
    img = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    total = img.astype(np.int64).reshape(2, 3, 2, 4, 3).sum((1, 3))
    want = np.rint(total.astype(np.float32) * np.float32(1.0 / 12)).astype(np.uint8)
    assert np.array_equal(RC.host_resize_image(L, img, 2, 2, "area"), want)


def test_area_table_weights_sum_to_one(L):
    """every (s, d) with d <= s <= 64: the entries of a destination index lie inside the source, ascend by one, and their weights
    sum to 1 within 1e-6; the numpy table is the same table"""
    idx, wt = np.zeros(80, np.int32), np.zeros(80, np.float32)
    worst = 0.0
    for s in range(1, 65):
        for d in range(1, s + 1):
            tab = RC.np_area_table(s, d)
            for i in range(d):
                n = L.resize_area_span_emul(i, s, d, 80, P(idx), P(wt))
                assert 1 <= n <= 80 and idx[0] >= 0 and idx[n - 1] <= s - 1 and (np.diff(idx[:n]) == 1).all(), (s, d, i)
                total = float(wt[:n].astype(np.float64).sum())
                worst = max(worst, abs(total - 1.0))
                assert abs(total - 1.0) <= 1e-6, (s, d, i, total)
                assert [(int(a), float(b)) for a, b in zip(idx[:n], wt[:n])] == [(a, float(b)) for a, b in tab[i]], (s, d, i)
    print("AREA table: largest |sum of weights - 1| = %.3g" % worst)


# ---- records --------------------------------------------------------------------------------------------------------------------------

SIZE_PAIRS = [((640, 480), (1280, 960)), ((1920, 1080), (3840, 2160)), ((1280, 720), (3840, 2160)), ((640, 480), (1000, 333)), ((3, 5), (32767, 1))]


def test_record_map_against_numpy(L):
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(-50, 4000, 4000), [0.0, -0.5, 0.25, 1e30, -1e30, np.inf, -np.inf, np.nan]]).astype(np.float32)
    for (sw, sh), (dw, dh) in SIZE_PAIRS:
        for s, d in ((sw, dw), (sh, dh), (dw, sw), (dh, sh)):
            got = np.zeros_like(p)
            L.resize_coords_emul(P(p), p.size, s, d, P(got))
            want = RC.np_scale_coords(p, s, d)
            assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (s, d)
    assert RC.np_scale_coords(np.float32([np.nan]), 2, 4).view(np.uint32)[0] == 0x7FC00000


def test_records_of_equal_sizes_are_copied_bit_for_bit(L):
    rng = np.random.default_rng(6)
    recs = np.frombuffer(rng.integers(0, 256, 3 * 4 * FK.MARKER_DTYPE.itemsize, dtype=np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(3, 4).copy()
    out = RC.host_scale_records(L, recs, [4, 2, 0], (640, 480), (640, 480))
    assert out.tobytes() == recs.tobytes()
    # one axis equal: its coordinates are copied, the other axis moves, nothing else does
    out = RC.host_scale_records(L, recs, [4, 2, 0], (640, 480), (640, 960))
    assert out["square"][0][:, 0::2].tobytes() == recs["square"][0][:, 0::2].tobytes()
    assert out["square"][0].view(np.uint32).tolist() == RC.np_scale_squares(recs["square"][0], (640, 480), (640, 960)).view(np.uint32).tolist()
    assert out[1, 2:].tobytes() == recs[1, 2:].tobytes() and out[2].tobytes() == recs[2].tobytes()
    for name in ("glMatrix", "templateId", "markerId", "score", "aspectRatio"):
        assert out[name].tobytes() == recs[name].tobytes()


def test_records_up_and_down_return(L):
    """each map rounds once to float32, at magnitudes of at most max(|p|, |up|) (and the offsets of 0.5 put a floor of 1 under
    that): the way there and back is within 1 ulp of that scale"""
    rng = np.random.default_rng(7)
    p = rng.uniform(-20, 2200, 20000).astype(np.float32)
    for small, large in SIZE_PAIRS[:4]:
        for s, d in zip(small, large):
            up, back = np.zeros_like(p), np.zeros_like(p)
            L.resize_coords_emul(P(p), p.size, s, d, P(up))
            L.resize_coords_emul(P(up), p.size, d, s, P(back))
            tol = np.spacing(np.maximum(np.maximum(np.abs(p), np.abs(up)), np.float32(1)))
            assert (np.abs(back.astype(np.float64) - p) <= tol).all(), (s, d)


# ---- the chain -------------------------------------------------------------------------------------------------------------------------

def chain_on_the_host(L):
    """per scene: (scene, full-size markers, small-size markers, their squares mapped up by the host core)"""
    tpls = RC.chain_templates()
    (W, Hh), (FW, FH) = RC.CHAIN_SMALL, RC.CHAIN_FULL
    out = []
    for sc in RC.chain_scenes():
        full, _, _ = H.oracle_registration(sc.frame, tpls, PS.camera(FW, FH))
        small_frame = RC.host_resize_image(L, sc.frame, W, Hh, "area")
        small, _, _ = H.oracle_registration(small_frame, tpls, PS.camera(W, Hh))
        recs = np.zeros((1, max(len(small), 1)), FK.MARKER_DTYPE)
        for k, m in enumerate(small):
            recs[0, k] = np.frombuffer(bytes(m), FK.MARKER_DTYPE)[0]
        up = RC.host_scale_records(L, recs, [len(small)], (W, Hh), (FW, FH))
        out.append((sc, full, small, up[0]))
    return out


def test_the_chain_on_the_cpu(L):
    """single planted markers on 1280 x 960 frames, shrunk by 2 with the host core and detected by the oracle at 640 x 480 with
    the camera of that size: the planted marker is found on the full frame and on the shrunk frame, with the same template, and
    the squares mapped back up lie within persp_synth.match's 6 px of the full-size detection and of the planted corners.
    Measured: at most 2.92 px from the full-size detection and 2.08 px from the planted corners (the full-size detection itself:
    1.41 px)."""
    worst_full = worst_truth = 0.0
    for sc, full, small, up in chain_on_the_host(L):
        assert len(full) == 1 and len(small) == 1, (sc.name, len(full), len(small))
        planted = sc.markers[0]
        m_full, k_full, d_full = PS.match(np.array(full[0].square), sc.markers)
        assert m_full is planted and k_full is not None, (sc.name, d_full)
        assert small[0].templateId == full[0].templateId == planted.template and small[0].score > 0
        m_up, k_up, d_truth = PS.match(up["square"][0], sc.markers)
        assert m_up is planted and k_up is not None, (sc.name, d_truth)
        d = RC.best_corner_distance(up["square"][0], np.array(full[0].square))
        print("%s: mapped-back corners %.2f px from the full-size detection, %.2f px from the planted corners (full size: %.2f px)" % (
            sc.name, d, d_truth, d_full))
        worst_full, worst_truth = max(worst_full, d), max(worst_truth, d_truth)
    print("chain: at most %.2f px from the full-size detection, %.2f px from the planted corners" % (worst_full, worst_truth))
    assert worst_full <= 6.0 and worst_truth <= 6.0


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers():
    """tests/emul/resize_emul.cpp with its own main, built with -fsanitize=address,undefined and run as a program: the sweep's
    extremes (sides 1 .. 32767, every pixel size and mode) on heap blocks of exactly the bytes a call may touch"""
    run_sanitized("resize_emul", "RESIZE_EMUL_MAIN", ", 0 bad", timeout=600)

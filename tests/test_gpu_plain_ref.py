"""GPU tests of the frame pass and the crop pass against tests/plain_ref.py, the plain second reference (numpy, scipy, rationals).
The oracle takes no part in the assertions: planes, border starts, squares, crop rectangles, crop planes and crop squares of the
kernels are held to the plain reference directly, on the fixed scenes of tests/plain_ref_scenes.py -- the smallest sizes that
reach each way the frame kernel cuts its work, which the host build of the batch plan confirms."""
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import plain_ref as R
import plain_ref_scenes as PS
from frame_kit import oa  # noqa: F401
from test_batch_plan_cpu import lib, plan   # noqa: F401  (lib: the fixture that builds tests/emul/plan_emul.cpp)
from test_gpu_parity import make_detector

pytestmark = pytest.mark.gpu

BATCH = 12            # frames at positions >= 8: from nine frames on the ring-quads kernels run
MARCH_STRIP = 240     # kernels.h
CROP_SIZES = [(320, 240), (496, 270)]   # the scenes that hold every drawn item
# the last strip's columns each size is there for (None: one strip)
LAST_STRIP = {(242, 48): 2, (244, 48): 4, (256, 48): 16, (241, 40): None, (481, 40): 240, (496, 270): 16, (320, 240): 80}


def size(w, h):
    return SimpleNamespace(width=w, height=h)


def ids(sizes):
    return ["%dx%d" % s for s in sizes]


def check_plan(lib, W, Hh, n):   # noqa: F811
    """the cut of the frame kernel's work that the size is in the list for"""
    p = plan(lib, W, Hh, n, max_batch=max(n, BATCH))
    assert (p.sw, p.sh) == (W & ~1, Hh & ~1)
    assert p.frame_strips == (p.sw + MARCH_STRIP - 1) // MARCH_STRIP
    if (W, Hh) in LAST_STRIP:
        last = p.sw - (p.frame_strips - 1) * MARCH_STRIP
        assert (None if p.frame_strips == 1 else last) == LAST_STRIP[(W, Hh)], (W, Hh, p.frame_strips, last)
    return p


class Plain:
    """the plain reference's planes of one BGR frame"""

    def __init__(self, bgr):
        self.grey = R.grey(bgr, "bgr")
        self.binary = R.binarise(self.grey)[0]
        self.masks = H.neighbour_masks(self.binary)


def check_planes(det, f, ref, where):
    h, w = ref.grey.shape
    assert np.array_equal(det.debug_gray(f, w, h), ref.grey), ("grey plane", where, f)
    assert np.array_equal(det.debug_binary(f, w, h)[1:-1, 1:-1], ref.binary[1:-1, 1:-1]), ("binary image", where, f)
    assert np.array_equal(det.debug_masks(f, w, h), ref.masks), ("mask plane", where, f)


def batch_of(frames, fmt, which):
    """[len(which)] frames in fmt: frames[k] for k in which"""
    return np.ascontiguousarray(np.stack([PS.in_format(frames[k], fmt, seed=i) for i, k in enumerate(which)]))


@pytest.mark.parametrize("W,Hh", PS.SIZES, ids=ids(PS.SIZES))
def test_planes_in_every_format(oa, lib, W, Hh):   # noqa: F811
    """grey, binary and mask planes of four distinct frames -- the scene, mirrored, upside down, noise -- at all twelve positions
    of a batch and as one-frame calls, in the five input formats, on one detector"""
    check_plan(lib, W, Hh, BATCH)
    check_plan(lib, W, Hh, 1)
    frames = PS.variants(PS.scene(W, Hh))
    refs = [Plain(b) for b in frames]
    for fmt in PS.FORMATS:
        assert np.array_equal(R.grey(PS.in_format(frames[0], fmt), fmt), refs[0].grey)   # (the formats carry the same colours)
    det, _, _ = make_detector(oa, size(W, Hh), None, BATCH)
    which = [k % 4 for k in range(BATCH)]
    for fmt in PS.FORMATS:
        det.set_input_format(fmt)
        det.detect_host(batch_of(frames, fmt, which))
        for f, k in enumerate(which):
            check_planes(det, f, refs[k], (W, Hh, fmt, "batch"))
        for k in (0, 3):
            det.detect_host(batch_of(frames, fmt, [k]))
            check_planes(det, 0, refs[k], (W, Hh, fmt, "one frame", k))
    det.close()


@pytest.mark.parametrize("W,Hh", PS.SIZES, ids=ids(PS.SIZES))
def test_starts_hold_every_start_of_the_labels(oa, W, Hh):
    """the start list the binarise kernel hands to the followers holds the first pixel of every component of the plain
    reference's binary image -- ones 8-connected, zeros 4-connected, a hole at its own first pixel -- with its hole flag"""
    frames = PS.variants(PS.scene(W, Hh))
    want = [{s | h << 31 for s, h in R.borders(R.binarise(R.grey(b, "bgr"))[0])} for b in frames]
    det, _, _ = make_detector(oa, size(W, Hh), None, BATCH)
    for which in ([k % 4 for k in range(BATCH)], [0], [3]):
        det.detect_host(batch_of(frames, "bgr", which))
        s = det.debug_starts(False)
        sw = W & ~1
        codes = (s["y"].astype(np.int64) * sw + s["x"]) | (s["is_hole"].astype(np.int64) << 31)
        for f, k in enumerate(which):
            got = set(codes[s["roi"] == f].tolist())
            assert want[k] <= got, (W, Hh, len(which), f, sorted(want[k] - got)[:8])
    det.close()


def plain_squares(bgr):
    sq, starts, undecided = R.find_squares(R.grey(bgr, "bgr"))
    assert not undecided, "the fixed scenes hold no knife edge"
    return sq


def same_squares(got, want, where):
    got = np.asarray(got, np.int64).reshape(-1, 4, 2)
    assert got.shape == want.shape and np.array_equal(got, want), ("squares", where, got.tolist(), want.tolist())


@pytest.mark.parametrize("W,Hh", PS.SIZES, ids=ids(PS.SIZES))
def test_squares_in_list_order(oa, W, Hh):
    """the squares of the frame pass after a batch on the device, and of the find_squares entry, equal the plain reference's
    in its order: the scene, its two mirror images and noise, at positions below and from 8 on"""
    import torch
    sc = PS.scene(W, Hh)
    frames = PS.variants(sc)
    want = [sc.squares[0]] + [plain_squares(b) for b in frames[1:]]
    assert not sc.squares[2] and (len(want[0]) >= 15 or (W, Hh) not in CROP_SIZES)
    det, _, _ = make_detector(oa, size(W, Hh), None, BATCH)
    which = [k % 4 for k in range(BATCH)]
    d = torch.from_numpy(batch_of(frames, "bgr", which)).cuda()
    det.detect_device(d.data_ptr(), W, Hh, BATCH)
    for f, k in enumerate(which):
        same_squares(det.debug_frame_quads(f), want[k], (W, Hh, "batch", f))
    d1 = torch.from_numpy(batch_of(frames, "bgr", [0])).cuda()
    det.detect_device(d1.data_ptr(), W, Hh, 1)
    same_squares(det.debug_frame_quads(0), want[0], (W, Hh, "one frame"))
    for k in range(4):
        got, n = det.find_squares(R.grey(frames[k], "bgr"))
        assert n == len(want[k])
        same_squares(got, want[k], (W, Hh, "find_squares", k))
    det.close()


@pytest.mark.parametrize("n", [1, 9], ids=["one_frame", "nine_frames"])
@pytest.mark.parametrize("W,Hh", CROP_SIZES, ids=ids(CROP_SIZES))
def test_crops_of_the_plain_squares(oa, W, Hh, n):
    """the crop pass: every crop's rectangle is crop_rect of the plain square that owns it, its binary image the plain binarise
    of the plain grey crop -- a second, smaller image with borders of its own -- and every candidate's patPoint the last square
    the plain reference finds in that crop"""
    sc = PS.scene(W, Hh)
    frames = PS.variants(sc)
    which = [(0, 1, 2)[k % 3] for k in range(n)]
    greys = [R.grey(b, "bgr") for b in frames]
    squares = [sc.squares[0]] + [plain_squares(b) for b in frames[1:3]]
    det, _, _ = make_detector(oa, size(W, Hh), None, n)
    det.detect_host(batch_of(frames, "bgr", which))
    rois = det.debug_crops()
    n_crops = n_cands = 0
    for f, k in enumerate(which):
        mine = rois[rois["frame"] == f]
        rects = [R.crop_rect(q, W, Hh) for q in squares[k]]
        with_plane = [i for i, (x0, y0, w, h) in enumerate(rects) if (w & ~1) >= 2 and (h & ~1) >= 2]
        assert sorted(int(r["owner"]) for r in mine) == with_plane, (W, Hh, n, f)
        last = {}
        for r in mine:
            x0, y0, w, h = rects[int(r["owner"])]
            assert (int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])) == (x0, y0, w, h), (W, Hh, n, f, int(r["owner"]))
            crop = greys[k][y0:y0 + h, x0:x0 + w]
            want = R.binarise(crop)[0]
            assert np.array_equal(det.debug_crop_binary(r)[1:-1, 1:-1], want[1:-1, 1:-1]), ("crop binary", W, Hh, n, f, int(r["owner"]))
            assert np.array_equal(det.debug_crop_masks(r), H.neighbour_masks(want)), ("crop masks", W, Hh, n, f, int(r["owner"]))
            sq, _, undecided = R.find_squares(crop)
            assert not undecided
            last[int(r["owner"])] = sq[-1] if len(sq) else None
            n_crops += 1
        cands = det.debug_candidates(f)
        # a square whose crop holds a square gives one candidate per template, in the squares' order
        assert [c.markerId for c in cands] == [i for i in with_plane if last[i] is not None for _ in range(det.n_templates)], (W, Hh, n, f)
        for c in cands:
            assert np.array_equal(np.array(c.patPoint), last[c.markerId].ravel().astype(np.float32)), ("patPoint", W, Hh, n, f, c.markerId)
            corners = np.array(c.square).reshape(4, 2).astype(np.int64)   # (the square, turned by the orientation it was read in)
            assert sorted(map(tuple, corners.tolist())) == sorted(map(tuple, squares[k][c.markerId].tolist())), ("square", W, Hh, n, f, c.markerId)
            n_cands += 1
    assert n_crops >= 15 * n and n_cands >= 15 * n, (n_crops, n_cands)
    det.close()


@pytest.mark.parametrize("knob,value", [("min_units", 1), ("mid_steps", 32)])
def test_follower_tiers_do_not_change_the_squares(oa, lib, knob, value):   # noqa: F811
    """496x270 in one chunk instead of two, and with tier 2's step budget at its least: borders change follower tiers, the
    squares stay the plain reference's"""
    W, Hh = 496, 270
    default, tuned = plan(lib, W, Hh, 1, max_batch=1), plan(lib, W, Hh, 1, max_batch=1, **{knob: value})
    assert (default.frame_strips, default.frame_chunks) == (3, 2)
    assert (tuned.frame_chunks, tuned.mid_steps) == ((1, default.mid_steps) if knob == "min_units" else (2, 32))
    assert default.mid_steps > 32
    sc = PS.scene(W, Hh)
    det, _, _ = make_detector(oa, size(W, Hh), None, 1)
    det.set_tuning(**{knob: value})
    det.detect_host(sc.bgr[None].copy())
    check_planes(det, 0, Plain(sc.bgr), (knob, value))
    same_squares(det.debug_frame_quads(0), sc.squares[0], (knob, value))
    got, n = det.find_squares(sc.grey)
    same_squares(got, sc.squares[0], (knob, value, "find_squares"))
    det.close()

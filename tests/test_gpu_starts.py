"""GPU tests of the border-start lists the binarise kernels hand to the followers (ocvar_hip_debug_starts): as sets they must be
what the border-start rule, evaluated pixel by pixel (tests/emul/starts_emul.cpp::se_rule) on the binary image the same kernel
wrote (debug_binary / debug_crop_binary), gives -- whichever way the frame is cut into strips, chunks and crop units, and also
for the frames of a batch that meet a busy memory system."""
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import work_cut_scenes as S
from frame_kit import oa  # noqa: F401
from helpers import P
from test_batch_plan_cpu import lib, plan   # noqa: F401  (lib: the fixture that builds tests/emul/plan_emul.cpp)
from test_gpu_parity import make_detector
from test_starts_cpu import build_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emul():
    return build_lib()


def rule_set(emul, binary):
    """the rule's starts of a binary image (0 / 255, the 1-px frame zero), as sorted y * w + x | hole << 31"""
    b = np.ascontiguousarray(binary)
    sh, sw = b.shape
    out = np.zeros(b.size + 1, np.uint32)
    n = emul.se_rule(P(b), sw, sh, P(out), out.size)
    assert 0 <= n <= out.size
    return np.sort(out[:n])


def list_sets(starts, widths):
    """a start list as {roi: sorted y * w + x | hole << 31}; no record twice, none outside its image"""
    sets = {}
    for roi, w in widths.items():
        s = starts[starts["roi"] == roi]
        assert ((s["x"] >= 0) & (s["x"] < w) & (s["y"] >= 0)).all(), roi
        assert ((s["is_hole"] == 0) | (s["is_hole"] == 1)).all(), roi
        codes = (s["y"].astype(np.int64) * w + s["x"]).astype(np.uint32) | (s["is_hole"].astype(np.uint32) << np.uint32(31))
        sets[roi] = np.sort(codes)
        assert len(np.unique(codes)) == len(codes), ("a start is listed twice", roi)
    assert set(np.unique(starts["roi"]).tolist()) <= set(widths), "a start of a ROI the batch does not have"
    return sets


def check_starts(det, emul, n_frames, W, Hh, where, min_crops=0, frames=None):
    """both start lists of det's last batch against the rule on the planes of the same batch; returns the crop records"""
    fs = det.debug_starts(False)
    assert len(fs) == int(det.counters()[0]) and len(fs) > 0, (where, len(fs), det.counters().tolist())
    got = list_sets(fs, {f: W & -2 for f in range(n_frames)})
    for f in (range(n_frames) if frames is None else frames):
        ref = rule_set(emul, det.debug_binary(f, W, Hh))
        assert got[f].shape == ref.shape and (got[f] == ref).all(), ("frame starts", where, f, len(got[f]), len(ref),
                                                                     np.setxor1d(got[f], ref)[:8].tolist())
    rois = det.debug_crops()
    assert len(rois) >= min_crops, (where, len(rois))
    cs = det.debug_starts(True)
    assert len(cs) == int(det.counters()[3]), (where, len(cs), det.counters().tolist())
    got = list_sets(cs, {int(r["index"]): int(r["w"]) & -2 for r in rois})
    for r in rois:
        if frames is not None and int(r["frame"]) not in frames:
            continue
        ref = rule_set(emul, det.debug_crop_binary(r))
        g = got[int(r["index"])]
        assert g.shape == ref.shape and (g == ref).all(), ("crop starts", where, [int(v) for v in r], len(g), len(ref),
                                                           np.setxor1d(g, ref)[:8].tolist())
    return rois


def size(w, h):
    return SimpleNamespace(width=w, height=h)


FW, FH = 496, 270   # three strips: an edge strip, an interior one, an edge strip of 16 columns; 270 rows: 19 tile rows and 4 rows


@pytest.mark.parametrize("min_units", [None, 1], ids=["two_chunks", "one_chunk"])
def test_starts_of_a_frame_with_edge_and_interior_strips(oa, emul, lib, min_units):   # noqa: F811
    p = plan(lib, FW, FH, 1, max_batch=1) if min_units is None else plan(lib, FW, FH, 1, max_batch=1, min_units=min_units)
    assert (p.frame_strips, p.frame_chunks) == (3, 2 if min_units is None else 1)
    frame = S.frame_of(FW, FH, 77, [(150, 40, 180), (400, 30, 60), (20, 100, 90)])
    det, _, _ = make_detector(oa, size(FW, FH), None, 1)
    if min_units is not None:
        det.set_tuning(min_units=min_units)
    det.detect_host(frame[None].copy())
    check_starts(det, emul, 1, FW, FH, ("496x270", min_units), min_crops=2)
    det.close()


def test_starts_of_a_crop_of_more_than_one_unit(oa, emul):
    W = Hh = 300
    frame = S.frame_of(W, Hh, 78, [(14, 16, 262)])
    det, _, _ = make_detector(oa, size(W, Hh), None, 1)
    det.detect_host(frame[None].copy())
    rois = check_starts(det, emul, 1, W, Hh, "tall crop", min_crops=1)
    assert max(int(r["h"]) & -2 for r in rois) > S.MARCH_CROP_ROWS   # (a start row in the second unit has its row above in the first)
    det.close()


def test_starts_of_every_frame_of_a_busy_batch(oa, emul):
    W, Hh, n = 640, 480, 64
    distinct = [S.frame_of(W, Hh, 90 + k, [(40 + 30 * k, 30 + 20 * k, 200 + 10 * k), (420, 300 - 40 * k, 70 + 8 * k)]) for k in range(4)]
    frames = np.stack([distinct[f % 4] for f in range(n)])
    det, _, _ = make_detector(oa, size(W, Hh), None, n)
    det.detect_host(frames)
    check_starts(det, emul, n, W, Hh, "64 x 640x480", min_crops=n)
    det.close()

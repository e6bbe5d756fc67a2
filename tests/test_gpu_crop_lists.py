"""The crop pass with lists that hold only what a phase walks and a step budget that fits the crop (follow.hip:
crop_split_kernel / crop_prune_kernel, follow_mid_kernel<true>; croplist_core.h), against the oracle: markers and decoded candidates of batches
of more than 8 frames of 640 x 480 (two phases, the lists and the crop budget in force) and of the same frames as one 8-frame
batch (one phase, neither).

What makes each scene the case it is meant to be -- the length of a crop's longest border, set against tier 2's budgets -- is
measured on the CPU with the oracle's contours (tests without the gpu mark); the GPU tests then read the tiers' list counters."""
import numpy as np
import pytest

import helpers as H
import test_gpu_parity as T
from frame_kit import oa  # noqa: F401

W, HH = 640, 480
MID_STEPS, CAP, BLOCK = 1536, 3072, 32   # kernels.h: MID_STEPS, CROP_STEPS_CAP; follow.hip: MID_BLOCK


def budget(cw, ch):
    """croplist_core.h::crop_walk_budget of a throughput batch for a crop of cw x ch pixels"""
    b = -(-6 * ((cw & ~1) + (ch & ~1)) // BLOCK) * BLOCK
    return min(CAP, max(MID_STEPS, b))


def border_steps(pts):
    """steps of the follower round a border given by its corner points (between two of them it runs straight: one pixel per step)"""
    p = np.asarray(pts, np.int64)
    return int(np.abs(p - np.roll(p, -1, axis=0)).max(axis=1).sum()) if len(p) > 1 else 0


def crops_of(bgr):
    """the crops the second pass makes of a frame, as the reference does (cvarSquare2Rect grown by 5 px, clipped): for each
    (width, height, quads found in it, its borders' lengths in steps, longest first)"""
    grey = np.ascontiguousarray(H.oracle_registration(bgr, H.oracle_templates(), H.oracle_camera(W, HH))[2][..., 0])
    out = []
    for q in H.oracle_find_squares(grey):
        x0, y0 = max(int(q[:, 0].min()) - 5, 0), max(int(q[:, 1].min()) - 5, 0)
        x1, y1 = min(int(q[:, 0].max()) + 5, W), min(int(q[:, 1].max()) + 5, HH)
        if ((x1 - x0) & ~1) < 2 or ((y1 - y0) & ~1) < 2:
            continue
        crop = np.ascontiguousarray(grey[y0:y1, x0:x1])
        borders, _, _ = H.oracle_contours(H.oracle_binarise(crop))
        out.append((x1 - x0, y1 - y0, len(H.oracle_find_squares(crop)), sorted((border_steps(b) for b in borders), reverse=True)))
    return out


# ---- the scenes -------------------------------------------------------------------------------------------------------------
def big_marker_frames():
    """(a) one marker of ~230 px a side at any rotation: the crop of its inner quad holds no quad, and its own frame border,
    merged with the marker's edge where the two touch, is longer than MID_STEPS"""
    cfg = H.synth_config(3, width=W, height=HH, grid_x=1, grid_y=1, side_min=225, side_max=235, rot_mode=1)
    return [H.synth_frame(cfg, s)[0] for s in (1, 2)] + \
           [H.synth_frame(H.synth_config(3, width=W, height=HH, grid_x=1, grid_y=1, side_min=225, side_max=235, rot_mode=0), 2)[0]]


def serpentine_frame(flip=False):
    """(b) a marker-sized square -- a dark ring of 200 px -- holding a dark serpentine line: 15 runs of 144 px, 10 px apart,
    joined at alternating ends.  The line's border is far longer than any tier-2 budget."""
    img = np.full((HH, W), 215, np.uint8)
    s, ring, lw, pitch, m = 200, 14, 3, 10, 14
    x0, y0 = (W - s) // 2, (HH - s) // 2
    img[y0:y0 + s, x0:x0 + s] = 25
    img[y0 + ring:y0 + s - ring, x0 + ring:x0 + s - ring] = 215
    xa, xb, y1 = x0 + ring + m, x0 + s - ring - m, y0 + s - ring - m
    for k, y in enumerate(range(y0 + ring + m, y1 - lw + 1, pitch)):
        img[y:y + lw, xa:xb] = 25                                   # a run
        if y + pitch + lw <= y1:
            xc = xb - lw if k % 2 == 0 else xa
            img[y:y + pitch + lw, xc:xc + lw] = 25                  # the joint to the next run
    if flip:
        img = np.ascontiguousarray(img[::-1, ::-1])
    return np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))


def small_marker_frames(n):
    """(c) 24 markers of 40..60 px per frame: dozens of crops per frame, with and without a quad, side by side in the lists"""
    cfg = H.synth_config(3, width=W, height=HH, grid_x=6, grid_y=4, side_min=40, side_max=60, rot_mode=1, corner_jitter_pct=4)
    return [H.synth_frame(cfg, 50 + f)[0] for f in range(n)]


# ---- the scenes are what they claim (CPU) -----------------------------------------------------------------------------------
def test_scene_a_has_quadless_crops_whose_border_fits_only_the_crop_budget():
    for f in big_marker_frames():
        crops = crops_of(f)
        # a border of L steps closes within a budget b when L < b; one longer than MID_STEPS + BLOCK overran the old budget for sure
        assert any(nq == 0 and MID_STEPS + BLOCK < steps[0] < budget(cw, ch) for cw, ch, nq, steps in crops), crops
        assert all(steps[0] < budget(cw, ch) for cw, ch, nq, steps in crops), crops   # nothing is left for tier 3


def test_scene_b_has_a_border_beyond_every_tier_2_budget():
    for flip in (False, True):
        crops = crops_of(serpentine_frame(flip=flip))
        assert crops and all(150 <= cw <= 260 and 150 <= ch <= 260 for cw, ch, nq, steps in crops), crops   # marker-sized
        assert any(steps[0] > CAP + BLOCK for cw, ch, nq, steps in crops), crops


def test_scene_c_mixes_crops_with_and_without_a_quad():
    for f in small_marker_frames(3):
        crops = crops_of(f)
        assert len(crops) >= 30, len(crops)
        assert sum(nq > 0 for _, _, nq, _ in crops) >= 10 and sum(nq == 0 for _, _, nq, _ in crops) >= 10, [c[2] for c in crops]


# ---- against the oracle (GPU) -----------------------------------------------------------------------------------------------
def run_and_check(oa, distinct, n, refs=None):
    """a batch of n frames cycling through `distinct`; every position against the oracle's result for its frame.  Returns the
    detector's counters (ocvar_hip_counters) and the references."""
    import torch
    cfg = H.synth_config(3, width=W, height=HH)
    det, tpls, cam = T.make_detector(oa, cfg, None, n)
    refs = refs or [T.OracleFrame(f, tpls, cam, planes=False) for f in distinct]
    frames = np.ascontiguousarray(np.stack([distinct[k % len(distinct)] for k in range(n)]))
    d = torch.from_numpy(frames).cuda()
    markers, counts = det.detect_device(d.data_ptr(), W, HH, n)
    for k in range(n):
        ref = refs[k % len(distinct)]
        T.check_candidates(det, k, ref, where="batch of %d" % n)
        T.check_markers(k, ref, markers, counts, where="batch of %d" % n)
    return det.counters(), refs


@pytest.fixture(scope="module")
def kept():
    return {}   # the oracle's results of a scene, for the 8-frame run of the same frames


@pytest.mark.gpu
def test_a_long_merged_frame_border_closes_in_tier_2(oa, kept):
    frames = big_marker_frames()
    c, kept["a"] = run_and_check(oa, frames, 12)
    assert c[7] > 0          # tier 2 had crop starts
    assert c[9] == 0, c      # and handed none of them to tier 3: every border fits its crop's budget (the CPU test above)
    assert sum(len(r.cands) for r in kept["a"]) >= 3


@pytest.mark.gpu
def test_b_a_border_beyond_the_cap_still_goes_through_tier_3(oa, kept):
    frames = [serpentine_frame(), serpentine_frame(flip=True), big_marker_frames()[0]]
    c, kept["b"] = run_and_check(oa, frames, 9)
    assert c[9] >= 6, c      # the line's border in each of the 6 serpentine frames reached the wave tier


@pytest.mark.gpu
def test_c_many_crops_per_frame_fill_the_lists(oa, kept):
    frames = small_marker_frames(4)
    c, kept["c"] = run_and_check(oa, frames, 16)
    assert c[1] >= 16 * 30 and c[7] >= 2000, c   # crops, and tier-2 starts off the crops' frames: several chunks of the list kernels


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["a", "b", "c"])
def test_d_the_same_frames_as_one_8_frame_batch(oa, kept, scene):
    frames = {"a": big_marker_frames, "b": lambda: [serpentine_frame(), serpentine_frame(flip=True), big_marker_frames()[0]],
              "c": lambda: small_marker_frames(4)}[scene]()
    run_and_check(oa, frames, 8, refs=kept.get(scene))

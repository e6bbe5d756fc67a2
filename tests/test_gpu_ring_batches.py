"""GPU test of follow.hip::ring_quads_kernel<true>, which takes the crop ROIs of a batch 64 at a time: batches whose crop pass has
1, 63, 64, 65 and 130 ROIs -- a partial group, a full one, a group that spills into a second, and a third --, more than 8 frames
each so that the ring kernels run, with clean rings and rings with one hole mixed (tests/ring_batch_scenes.py).  A ring's verdict
shows in what it causes: a clean ring's start is dropped by tier 1 and its rectangle published by the ring kernel, a holed
ring's border is walked.  So the candidates and markers of every frame must be the oracle's, and the batch's work counters those
recorded for the same input from the kernels as they were when one wave took one ROI (tests/golden/ring_batches_counters.json).
That the scenes do hold both kinds of ring is asserted here on the CPU from the oracle alone."""
import json
import os

import numpy as np
import pytest

import helpers as H
import ring_batch_scenes as R
from frame_kit import oa  # noqa: F401
from test_gpu_parity import OracleFrame, check_candidates, check_markers, make_detector
from test_gpu_starts import size

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "ring_batches_counters.json")
# ocvar_hip_counters: frame starts, crop ROIs, crop tiles, crop starts, crop pixels, pool ints, tier-2 starts of the frame and the
# crop pass, tier-3 starts of the frame and the crop pass
N_COUNTERS = 10


@pytest.fixture(scope="module")
def oracle_frames():
    """the oracle's results and ring kinds per distinct frame of all scenes, computed once"""
    tpls, cam = H.oracle_templates(), H.oracle_camera(R.W, R.HH)
    cache = {}

    def get(frame):
        key = frame.tobytes()
        if key not in cache:
            ref = OracleFrame(frame, tpls, cam, planes=False)
            _, _, grey = H.oracle_registration(frame, tpls, cam)
            cache[key] = (ref, R.ring_kinds(frame, np.ascontiguousarray(grey[..., 0])))
        return cache[key]
    return get


@pytest.mark.parametrize("n_rois", R.COUNTS)
def test_crop_rings_in_groups_of_64(oa, oracle_frames, n_rois):
    frames, per = R.batch_of(n_rois)
    assert len(frames) > 8
    # the oracle alone: the batch has n_rois crops, their rings are clean or have exactly one hole, both kinds are there
    kinds = []
    for f, c in zip(frames, per):
        k = oracle_frames(f)[1]
        assert len(k) == c
        kinds += [holes for *_, holes in k]
    assert len(kinds) == n_rois and set(kinds) <= {0, 1}
    assert kinds.count(0) >= 1 and (n_rois == 1 or kinds.count(1) >= n_rois // 4), (kinds.count(0), kinds.count(1))

    det, _, _ = make_detector(oa, size(R.W, R.HH), None, len(frames))
    markers, counts = det.detect_host(frames.copy())
    assert len(det.debug_crops()) == n_rois
    n_cands = 0
    for f in range(len(frames)):
        ref = oracle_frames(frames[f])[0]
        check_candidates(det, f, ref, where=(n_rois, f))
        check_markers(f, ref, markers, counts, where=(n_rois, f))
        n_cands += len(ref.cands)
    assert n_cands >= 3 * n_rois   # (every crop's square is decoded against the three templates)
    got = det.counters(N_COUNTERS).tolist()
    want = json.load(open(GOLDEN))[str(n_rois)]
    assert got == want, (n_rois, got, want)
    det.close()

"""The device path on camera views (tests/persp_synth.py: tilt up to 75 degrees, markers at the frame's edge, frame sizes from
32x48 to 3840x2160, a wide-angle and a distorting camera): every scene against the oracle under the bars of
tests/test_gpu_parity.py, refinement at half windows 1 .. 15 against the host chain of tests/refine_chain.py, the device's
poses against the poses the markers were rendered from (the bounds of tests/test_perspective_cpu.py), find_squares on the
steepest frames."""
import numpy as np
import pytest

import helpers as H
import persp_synth as PS
import refine_chain as RC
import test_gpu_parity as GP
import test_perspective_cpu as TC
from frame_kit import oa  # noqa: F401

pytestmark = pytest.mark.gpu

REFINE_SETTINGS = [(1, 30, 0.1), (2, 30, 0.1), (5, 30, 0.1), (8, 30, 0.1), (15, 30, 0.1), (5, 1, 0.1)]
MIN_BATCH = 18   # scene frames also sit at batch positions >= 16


@pytest.fixture(scope="module")
def L():
    return RC.build_emul()


class Group:
    """the scenes of one frame size and camera as one device batch (tiled up to MIN_BATCH frames), its detector, and the
    oracle's results of each distinct scene"""

    def __init__(self, oa, scenes, tpls):
        import torch
        self.scenes, self.cam = scenes, scenes[0].cam
        self.w, self.h = scenes[0].width, scenes[0].height
        self.order = list(range(len(scenes)))
        while len(self.order) < MIN_BATCH:
            self.order += list(range(len(scenes)))
        self.n = len(self.order)
        self.det = oa.Detector(self.w, self.h, max_batch=self.n)
        self.det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
        self.det.set_camera(oa.Camera.from_buffer_copy(bytes(self.cam)))
        self.d = torch.from_numpy(np.stack([scenes[i].frame for i in self.order])).to("cuda:0")
        self.refs = [GP.OracleFrame(s.frame, tpls, s.cam) for s in scenes]

    def detect(self):
        return self.det.detect_device(self.d.data_ptr(), self.w, self.h, self.n)

    def last(self, i):
        """the last batch position that holds scene i"""
        return max(f for f, j in enumerate(self.order) if j == i)


@pytest.fixture(scope="module")
def groups(oa):
    tpls = H.oracle_templates(PS.NAMES)
    by_key = {}
    for s in PS.all_scenes():
        by_key.setdefault((s.width, s.height, bytes(s.cam)), []).append(s)
    return tpls, [Group(oa, sc, tpls) for sc in by_key.values()]


def test_every_scene_against_the_oracle_and_the_planted_poses(groups):
    """grey plane, binary image, frame quads, candidates bit-exact, markers exact, pose within POSE_RTOL (check_frame's checks
    with the oracle's results of a scene computed once); then the device's glMatrix against the planted poses under the CPU
    module's bounds"""
    tpls, gs = groups
    assert any(len({s.family for s in g.scenes}) >= 2 for g in gs)   # (one batch mixes families)
    assert any(s.lens for g in gs for s in g.scenes)
    table = {}
    n_markers = 0
    for g in gs:
        markers, counts = g.detect()
        for f, i in enumerate(g.order):
            ref = g.refs[i]
            where = g.scenes[i].name
            if f == g.last(i):
                GP.check_planes(g.det, f, ref, where)
            GP.check_candidates(g.det, f, ref, where)
            GP.check_markers(f, ref, markers, counts, where)
            if f != g.last(i):
                continue
            for k in range(int(counts[f])):
                m, shift, _ = PS.match(markers[f, k]["square"], g.scenes[i].markers)
                n_markers += 1
                if shift is None:
                    continue
                ang, rel = PS.truth_errors(markers[f, k]["glMatrix"], m, shift)
                w = table.setdefault((m.tilt, m.size >= TC.LARGE), [0.0, 0.0, 0])
                w[0], w[1], w[2] = max(w[0], ang), max(w[1], rel), w[2] + 1
    assert n_markers == sum(TC.FAMILY_COUNTS.values())
    TC.check_truth(table, 0, "device")


@pytest.mark.parametrize("setting", REFINE_SETTINGS)
def test_refinement_against_the_host_chain(groups, L, setting):
    """every scene -- the edge family, the panel-boundary frames and the 32x48 frame among them -- with refinement on: squares
    bit-exact with the host build of refine_core.h on the oracle's records, poses within the bar"""
    tpls, gs = groups
    moved = 0
    for g in gs:
        g.det.set_corner_refine(*setting)
        try:
            markers, counts = g.detect()
        finally:
            g.det.set_corner_refine(half_win=0)
        for f, i in enumerate(g.order):
            ref = g.refs[i]
            exp = RC.refined_markers(L, ref.markers, ref.grey, g.cam, setting)
            RC.check(markers, counts, f, exp, (g.scenes[i].name, setting))
            moved += RC.records_differ(exp, ref.markers)
    assert moved >= 50


def test_refined_edge_markers_through_the_host_entry_and_a_tracked_step(oa, groups, L):
    """the edge family through detect_host with refinement on, and one tracked step (enqueue_tracked) whose prev records are
    the refined edge markers"""
    import torch
    tpls, gs = groups
    g = [g for g in gs if any(s.family == "edges" for s in g.scenes)][0]
    idx = [i for i, s in enumerate(g.scenes) if s.family == "edges"]
    frames = np.stack([g.scenes[i].frame for i in idx])
    setting = (5, 30, 0.1)
    n = len(idx)
    det = oa.Detector(g.w, g.h, max_batch=n)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(g.cam)))
    det.set_corner_refine(*setting)
    markers, counts = det.detect_host(frames.copy())
    exp = [RC.refined_markers(L, g.refs[i].markers, g.refs[i].grey, g.cam, setting) for i in idx]
    for f in range(n):
        RC.check(markers, counts, f, exp[f], ("detect_host", g.scenes[idx[f]].name))
    assert sum(len(e) for e in exp) == TC.FAMILY_COUNTS["edges"]
    M = det.max_markers
    d_prev = torch.from_numpy(markers.view(np.uint8).reshape(n, M, -1).copy()).to("cuda:0")
    d_cnt = torch.from_numpy(np.minimum(counts, M).astype(np.int32)).to("cuda:0")
    d = torch.from_numpy(frames).to("cuda:0")
    det.enqueue_tracked(d.data_ptr(), g.w, g.h, n, d_prev.data_ptr(), d_cnt.data_ptr())
    m2, c2 = det.collect()
    tracked = 0
    for f in range(n):
        e2, _ = RC.expected(L, frames[f], tpls, g.cam, setting, prev=exp[f])
        RC.check(m2, c2, f, e2, ("enqueue_tracked", g.scenes[idx[f]].name))
        tracked += len(e2)
    assert tracked >= 1


def test_find_squares_on_the_steepest_frames(groups):
    tpls, gs = groups
    steep = PS.steepest()
    g = [g for g in gs if steep[0] in g.scenes][0]
    found = 0
    for s in steep:
        gray = g.refs[g.scenes.index(s)].grey
        ref = H.oracle_find_squares(gray)
        got, n = g.det.find_squares(gray)
        assert n == len(ref) and np.array_equal(got, ref), s.name   # (order included)
        found += n
    assert found >= 3 * len(steep)

"""Planar board pose (ocvar_hip_set_board) on the CPU: the host build of opencv-ar_amd/csrc/board_core.h against noise-free
projections, against an independent least-squares solver under noise, and against the ground truth of boards rendered with
ocvar_synth_draw_quads and detected by the oracle (the corner convention of include/ocvar_hip.h is pinned there)."""
import ctypes as C
import math

import numpy as np
import pytest

import board_chain as BC
import helpers as H
import refine_chain as RC
from helpers import P

SET5 = (5, 30, 0.1)


@pytest.fixture(scope="module")
def Lb():
    return BC.build_emul()


@pytest.fixture(scope="module")
def Lr():
    return RC.build_emul()


def camera(dist=False):
    cam = H.oracle_camera(1920, 1080)
    if dist:
        cam.distCoeffs[:] = [-0.12, 0.05, 0.0007, -0.0005, -0.01]
    return cam


def random_board(rng, n):
    """n markers of side 1 at random places and in-plane angles on a plane; template ids distinct"""
    tids = rng.choice(4096, n, replace=False)
    out = []
    for k in range(n):
        c = rng.uniform(-4, 4, 2)
        a = rng.uniform(0, 2 * math.pi)
        R2 = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        sq = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) @ R2.T + c
        out.append((int(tids[k]), sq))
    return out


def random_view(rng, board):
    R = BC.rodrigues(rng.normal(0, 1, 3) * 0.3) @ BC.rodrigues([0, 0, rng.uniform(0, 2 * math.pi)])
    t = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(14, 24)])
    return R, t


def solve_obs(Lb, board, sq, cam):
    """the core's solver on observations sq [n, 4, 2] (double) of every board entry"""
    ent = BC.entries(board)
    idx = np.arange(max(len(board), 1), dtype=np.int32)
    s = np.ascontiguousarray(np.asarray(sq, np.float64).reshape(-1, 8))
    if len(s) == 0:
        s = np.zeros((1, 8))
    out = BC.BoardPose()
    Lb.board_solve_obs(ent, P(idx), P(s), len(board), C.byref(cam), C.byref(out))
    return out


@pytest.mark.parametrize("dist", [False, True])
def test_noise_free_projections_recover_the_pose(Lb, dist):
    rng = np.random.default_rng(3 + dist)
    cam = camera(dist)
    K, dc = BC.cam_arrays(cam)
    for trial in range(40):
        n = [1, 2, 5, 16, 64][trial % 5]
        board = random_board(rng, n)
        R, t = random_view(rng, board)
        sq = np.stack([BC.project(K, dc, R, t, c) for _, c in board])
        pose = solve_obs(Lb, board, sq, cam)
        assert pose.status == 1 and pose.n_markers == n
        rv = BC.rvec_of(R)
        assert np.abs(np.array(pose.rvec) - rv).max() <= 1e-9 * max(1.0, np.linalg.norm(rv)), (trial, list(pose.rvec), rv)
        assert np.abs(np.array(pose.tvec) - t).max() <= 1e-9 * np.linalg.norm(t), (trial, list(pose.tvec), t)
        assert pose.rms < 1e-6


@pytest.mark.parametrize("dist", [False, True])
def test_noisy_projections_match_an_independent_solver(Lb, dist):
    from scipy.optimize import least_squares
    rng = np.random.default_rng(17 + dist)
    cam = camera(dist)
    K, dc = BC.cam_arrays(cam)
    for trial in range(20):
        n = [1, 3, 8, 32, 64][trial % 5]
        board = random_board(rng, n)
        R, t = random_view(rng, board)
        pts = np.concatenate([c for _, c in board])
        sq = np.stack([BC.project(K, dc, R, t, c) for _, c in board]) + rng.normal(0, 0.3, (n, 4, 2))
        pose = solve_obs(Lb, board, sq, cam)
        assert pose.status == 1

        def resid(x):
            return (BC.project(K, dc, BC.rodrigues(x[:3]), x[3:], pts) - sq.reshape(-1, 2)).ravel()

        ls = least_squares(resid, np.r_[BC.rvec_of(R), t], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        x = np.r_[pose.rvec, pose.tvec]
        assert np.abs(x - ls.x).max() <= 1e-6 * max(1.0, np.abs(ls.x).max()), (trial, x, ls.x)
        assert abs(pose.rms - math.sqrt(np.sum(ls.fun ** 2) / (4 * n))) <= 1e-6


def test_no_markers_and_degenerate_observations(Lb):
    cam = camera()
    board = random_board(np.random.default_rng(5), 2)
    pose = solve_obs(Lb, board[:0], np.zeros((0, 4, 2)), cam)
    assert pose.status == 0 and pose.n_markers == 0
    flat = np.zeros((2, 4, 2)) + 500.0   # every corner on one pixel: no homography
    pose = solve_obs(Lb, board, flat, cam)
    assert pose.status == -1 and pose.n_markers == 2


def test_set_board_rules(Lb):
    sq = [[0, 0], [1, 0], [1, 1], [0, 1]]

    def first_bad(entries):
        return Lb.board_first_bad_emul(BC.entries(entries), len(entries))

    assert first_bad([]) == -1
    assert first_bad([(0, sq), (4095, np.array(sq) + 2)]) == -1
    assert first_bad([(0, sq[::-1])]) == -1                          # either winding
    assert first_bad([(0, sq), (-1, sq)]) == 1
    assert first_bad([(0, sq), (4096, sq)]) == 1
    assert first_bad([(3, sq), (4, sq), (3, sq)]) == 2               # repeated template
    assert first_bad([(0, [[0, 0], [1, 0], [0, 1], [1, 1]])]) == 0   # self-intersecting
    assert first_bad([(0, [[0, 0], [1, 0], [2, 0], [0, 1]])]) == 0   # three corners on a line
    assert first_bad([(0, [[0, 0], [2, 0], [0.5, 0.5], [0, 2]])]) == 0   # concave
    assert first_bad([(0, [[0, 0], [0, 0], [0, 0], [0, 0]])]) == 0
    assert first_bad([(0, [[0, 0], [1, 0], [1, float("nan")], [0, 1]])]) == 0
    assert first_bad([(0, [[0, 0], [1, 0], [1, float("inf")], [0, 1]])]) == 0


def test_grid_board_layout():
    import opencv_ar_amd as oa
    b = oa.grid_board([7, 8, 9, 10, 11], 3, 2, 2.0, 0.5)
    assert [t for t, _ in b] == [7, 8, 9, 10, 11]
    assert np.array_equal(b[4][1], [[2.5, 2.5], [4.5, 2.5], [4.5, 4.5], [2.5, 4.5]])
    assert np.array_equal(b[2][1], [[5.0, 0.0], [7.0, 0.0], [7.0, 2.0], [5.0, 2.0]])
    for (t0, c0), (t1, c1) in zip(b, BC.grid_board([7, 8, 9, 10, 11], 3, 2, 2.0, 0.5)):
        assert t0 == t1 and np.array_equal(c0, c1)
    with pytest.raises(ValueError):
        oa.grid_board(list(range(7)), 3, 2, 1.0, 0.1)


N_SCENES = 24


@pytest.fixture(scope="module")
def rendered():
    names, board, sc = BC.scenes(N_SCENES)
    return dict(names=names, board=board, scenes=sc, tpls=H.oracle_templates(names), cam=H.oracle_camera(1920, 1080))


@pytest.mark.parametrize("refine", [SET5, None])
def test_rendered_boards_against_ground_truth(Lb, Lr, rendered, refine):
    board, tpls, cam = rendered["board"], rendered["tpls"], rendered["cam"]
    worst = [0.0, 0.0, 0.0]
    rots = set()
    for i, (bgr, truth, R, t) in enumerate(rendered["scenes"]):
        ref, gray, pose, first, rot = BC.expected(Lr, Lb, bgr, board, tpls, cam, refine)
        # every planted marker is used, and the rotation read on it is the one that lines its record corners up with the
        # truth's corners 0..3 (the corner convention)
        assert pose.status == 1 and pose.n_markers == len(board), (i, pose.n_markers, first.tolist(), rot.tolist())
        for b in range(len(board)):
            k, d = BC.truth_shift(ref[first[b]].square, truth[b])
            assert rot[b] == k and d < 6.0, (i, b, rot[b], k, d)
            rots.add(int(k))
        ang, rel = BC.pose_errors(pose, R, t)
        worst = [max(worst[0], ang), max(worst[1], rel), max(worst[2], pose.rms)]
    print("\nboard vs truth, refine %s: worst rotation %.3f deg, translation %.5f of distance, rms %.3f px"
          % (refine, *worst))
    assert len(rots) >= 2   # the records of these scenes start at different corners
    if refine:
        assert worst[0] <= 0.5 and worst[1] <= 0.01 and worst[2] <= 1.0, worst
    else:
        assert worst[0] <= 1.0 and worst[1] <= 0.02 and worst[2] <= 2.0, worst


def test_first_record_of_each_entry_and_score_zero_ignored(Lb, rendered):
    """a duplicate of a record later in output order is never chosen; a record with score 0 never serves its template"""
    board, tpls, cam = rendered["board"], rendered["tpls"], rendered["cam"]
    bgr, truth, R, t = rendered["scenes"][0]
    ref, _, img = H.oracle_registration(bgr, tpls, cam)
    gray = np.ascontiguousarray(img[:, :, 0])
    p0, f0, r0 = BC.host_board(Lb, gray, ref, board, tpls, cam)
    dup = H.Marker.from_buffer_copy(bytes(ref[0]))
    dup.square[:] = [v + 40.0 for v in dup.square]
    p1, f1, r1 = BC.host_board(Lb, gray, list(ref) + [dup], board, tpls, cam)
    assert bytes(p0) == bytes(p1) and np.array_equal(f0, f1)
    zero = H.Marker.from_buffer_copy(bytes(ref[0]))
    zero.score = 0.0
    p2, f2, r2 = BC.host_board(Lb, gray, [zero] + list(ref[1:]), board, tpls, cam)
    b0 = [b for b, (tid, _) in enumerate(board) if tid == ref[0].templateId][0]
    assert f2[b0] == -1 and p2.n_markers == len(board) - 1

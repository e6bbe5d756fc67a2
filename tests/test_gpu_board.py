"""Planar board pose on the device (ocvar_hip_set_board) against the host build of board_core.h run on the device's own
records and grey planes (tests/board_chain.py): counts and status exactly, poses within 1e-6; and against the ground truth of
the rendered boards."""
import ctypes as C

import numpy as np
import pytest

import board_chain as BC
import dense_synth as DS
import helpers as H
from frame_kit import oa  # noqa: F401

pytestmark = pytest.mark.gpu

SET5 = (5, 30, 0.1)
N = 64
W_, H_ = 1920, 1080
RTOL = 1e-6


@pytest.fixture(scope="module")
def Lb():
    return BC.build_emul()


@pytest.fixture(scope="module")
def scene():
    names, board, sc = BC.scenes(N)
    return dict(names=names, board=board, frames=np.stack([s[0] for s in sc]), truth=[s[1:] for s in sc],
                tpls=H.oracle_templates(names), cam=H.oracle_camera(W_, H_))


def device_frames(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames)).to("cuda:0")


def detector(oa, tpls, cam, n, board=None, **kw):
    det = oa.Detector(W_, H_, max_batch=n, **kw)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    if board is not None:
        det.set_board(board)
    return det


def records(markers, counts, f):
    return [H.Marker.from_buffer_copy(markers[f, k].tobytes()) for k in range(min(int(counts[f]), markers.shape[1]))]


def found_templates(markers, counts, f):
    """the templates of frame f's records with score > 0 (what the board may use)"""
    return {int(m["templateId"]) for m in markers[f, :min(int(counts[f]), markers.shape[1])] if m["score"] > 0}


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= RTOL * max(1.0, np.abs(b).max())


def check_against_host(Lb, det, markers, counts, poses, board, tpls, cam, frames=None, where=""):
    """every frame's device pose against the host core on the device's records and grey plane; returns the host poses"""
    out = []
    for f in range(len(poses)) if frames is None else frames:
        gray = det.debug_gray(f, W_, H_)
        hp, first, rot = BC.host_board(Lb, gray, records(markers, counts, f), board, tpls, cam)
        p = poses[f]
        assert (p["status"], p["n_markers"]) == (hp.status, hp.n_markers), (where, f, p["status"], p["n_markers"], hp.status, hp.n_markers)
        assert hp.n_markers == int((rot >= 0).sum())
        if hp.status == 1:
            assert close(p["glMatrix"], hp.glMatrix) and close(p["rvec"], hp.rvec) and close(p["tvec"], hp.tvec), (where, f)
            assert abs(p["rms"] - hp.rms) <= RTOL * max(1.0, hp.rms)
        out.append(hp)
    return out


@pytest.mark.parametrize("refine", [SET5, None])
def test_batch_of_64_against_host_core_and_truth(oa, Lb, scene, refine):
    det = detector(oa, scene["tpls"], scene["cam"], N, scene["board"])
    if refine:
        det.set_corner_refine(*refine)
    d = device_frames(scene["frames"])
    markers, counts = det.detect_device(d.data_ptr(), W_, H_, N)
    poses = det.board_poses()
    assert poses.shape == (N,) and poses.dtype == oa.BOARD_DTYPE
    check_against_host(Lb, det, markers, counts, poses, scene["board"], scene["tpls"], scene["cam"], where=refine)
    worst = [0.0, 0.0, 0.0]
    complete = 0
    for f in range(N):
        p = poses[f]
        # every board marker the detector found is used (it misses one now and then: the reference's readout, not the board's)
        assert p["status"] == 1 and p["n_markers"] == len(found_templates(markers, counts, f)), (f, p["status"], p["n_markers"])
        complete += int(p["n_markers"]) == len(scene["board"])
        R, t = scene["truth"][f][1], scene["truth"][f][2]
        pose = BC.BoardPose.from_buffer_copy(p.tobytes())
        ang, rel = BC.pose_errors(pose, R, t)
        worst = [max(worst[0], ang), max(worst[1], rel), max(worst[2], float(p["rms"]))]
    print("\ndevice board vs truth, refine %s: worst rotation %.3f deg, translation %.5f of distance, rms %.3f px; all %d markers "
          "in %d of %d frames" % (refine, *worst, len(scene["board"]), complete, N))
    assert complete >= N - 4
    if refine:
        assert worst[0] <= 0.5 and worst[1] <= 0.01 and worst[2] <= 1.0, worst
    else:
        assert worst[0] <= 1.0 and worst[1] <= 0.02 and worst[2] <= 2.0, worst


def test_distorted_camera(oa, Lb):
    cam = H.oracle_camera(W_, H_)
    cam.distCoeffs[:] = [-0.08, 0.03, 0.0005, -0.0004, 0.0]
    names, board, sc = BC.scenes(16, seed=5, cam=cam)   # (rendered through the distorted camera)
    frames = np.stack([s[0] for s in sc])
    tpls = H.oracle_templates(names)
    det = detector(oa, tpls, cam, 16, board)
    det.set_corner_refine(*SET5)
    d = device_frames(frames)
    markers, counts = det.detect_device(d.data_ptr(), W_, H_, 16)
    poses = det.board_poses()
    check_against_host(Lb, det, markers, counts, poses, board, tpls, cam, where="dist")
    for f in range(16):
        assert poses[f]["status"] == 1
        ang, rel = BC.pose_errors(BC.BoardPose.from_buffer_copy(poses[f].tobytes()), sc[f][2], sc[f][3])
        assert ang <= 0.5 and rel <= 0.01, (f, ang, rel)


def test_board_changes_no_marker_and_no_count(oa, scene):
    d = device_frames(scene["frames"][:16])
    plain = detector(oa, scene["tpls"], scene["cam"], 16)
    m0, c0 = plain.detect_device(d.data_ptr(), W_, H_, 16)
    with pytest.raises(oa.OcvarError):
        plain.board_poses()   # no board: no poses
    det = detector(oa, scene["tpls"], scene["cam"], 16, scene["board"])
    m1, c1 = det.detect_device(d.data_ptr(), W_, H_, 16)
    assert np.array_equal(c0, c1) and m0.tobytes() == m1.tobytes()
    assert (det.board_poses()["status"] == 1).all()
    det.set_board(None)
    m2, c2 = det.detect_device(d.data_ptr(), W_, H_, 16)
    assert np.array_equal(c0, c2) and m0.tobytes() == m2.tobytes()
    with pytest.raises(oa.OcvarError):
        det.board_poses()


def test_frames_without_board_markers(oa, scene):
    """config-3 frames carry the shipped templates only, and a blank frame carries nothing: status 0, no marker used"""
    cfg = H.synth_config(3)
    frames = np.stack([H.synth_frame(cfg, f)[0] for f in range(3)] + [np.full((H_, W_, 3), 220, np.uint8)])
    tpls = H.oracle_templates(H.TEMPLATE_ORDER + scene["names"])
    board = [(t + len(H.TEMPLATE_ORDER), c) for t, c in scene["board"]]
    det = detector(oa, tpls, scene["cam"], 4, board)
    d = device_frames(frames)
    markers, counts = det.detect_device(d.data_ptr(), W_, H_, 4)
    assert counts[:3].min() > 0
    poses = det.board_poses()
    assert (poses["status"] == 0).all() and (poses["n_markers"] == 0).all()
    assert not poses["glMatrix"].any() and not poses["rvec"].any() and not poses["tvec"].any()


def test_tracked_steps_take_part(oa, Lb, scene):
    """three enqueue_tracked steps over the same frames, each step's records the next step's prev: the board uses the records
    the tracking stage hands on, as the host core does on the same records"""
    import torch
    S = 8
    det = detector(oa, scene["tpls"], scene["cam"], S, scene["board"])
    det.set_corner_refine(*SET5)
    M = det.max_markers
    d_prev = torch.zeros((S, M, oa.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    d = device_frames(scene["frames"][:S])
    for step in range(3):
        det.enqueue_tracked(d.data_ptr(), W_, H_, S, d_prev.data_ptr(), d_cnt.data_ptr())
        m, c = det.collect()
        poses = det.board_poses()
        check_against_host(Lb, det, m, c, poses, scene["board"], scene["tpls"], scene["cam"], where=("tracked", step))
        assert (poses["status"] == 1).all()
        assert [int(p) for p in poses["n_markers"]] == [len(found_templates(m, c, s)) for s in range(S)]
        assert all(len(found_templates(m, c, s)) > 0 for s in range(S))
        d_prev.copy_(torch.from_numpy(m.view(np.uint8).reshape(S, M, -1)).to("cuda:0"))
        d_cnt.copy_(torch.from_numpy(np.minimum(c, M).astype(np.int32)).to("cuda:0"))


def dense_frame(cfg, names):
    """frame 0 of cfg with its truth for every planted marker (helpers.synth_frame keeps at most 256)"""
    tp = H.template_pixels()
    arrs = [np.ascontiguousarray(tp[n][0]) for n in names]
    st = (H.SynthTemplate * len(arrs))()
    for i, a in enumerate(arrs):
        st[i].pixels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        st[i].h, st[i].w = a.shape
    bgr = np.zeros((cfg.height, cfg.width, 3), np.uint8)
    truth = (H.SynthMarker * (cfg.grid_x * cfg.grid_y))()
    n = H.synth_lib().ocvar_synth_frame(C.byref(cfg), 0, st, len(arrs), H.P(bgr), cfg.width * 3, truth, len(truth))
    return bgr, [dict(corner=np.array(truth[i].corner).reshape(4, 2), template=truth[i].template_index) for i in range(n)]


def test_dense_context_with_a_256_marker_board(oa, Lb):
    """312 upright markers of tests/dense_synth.py on a dense context; the board is 256 of them, with board coordinates that
    put the frame's marker corners on the plane z = 10 seen by the camera at the identity pose"""
    names = DS.library(24 * 13)
    cfg = DS.config(W_, H_, 24, 13)
    bgr, truth = dense_frame(cfg, names)
    cam = H.oracle_camera(W_, H_)
    K, _ = BC.cam_arrays(cam)
    Z = 10.0
    board = []
    for m in truth:
        if m["template"] < 256:
            uv = m["corner"] - 0.5
            board.append((m["template"], np.c_[(uv[:, 0] - K[0, 2]) / K[0, 0] * Z, (uv[:, 1] - K[1, 2]) / K[1, 1] * Z]))
    assert len(board) == 256
    n = 4
    tpls = H.oracle_templates(names)
    det = detector(oa, tpls, cam, n, board, max_quads=1024, max_markers=512)
    d = device_frames(np.stack([bgr] * n))
    markers, counts = det.detect_device(d.data_ptr(), W_, H_, n)
    poses = det.board_poses()
    check_against_host(Lb, det, markers, counts, poses, board, tpls, cam, frames=[0, 3], where="dense")
    assert (poses["n_markers"] == 256).all() and (poses["status"] == 1).all()
    assert np.abs(poses["rvec"]).max() < 2e-3 and np.abs(poses["tvec"] - [0, 0, Z]).max() < 0.02 * Z


def test_detect_host_covers_every_frame(oa, scene):
    n = 20
    frames = np.ascontiguousarray(scene["frames"][:n])
    ref = detector(oa, scene["tpls"], scene["cam"], n, scene["board"])
    d = device_frames(frames)
    ref.detect_device(d.data_ptr(), W_, H_, n)
    want = ref.board_poses()
    det = detector(oa, scene["tpls"], scene["cam"], 8, scene["board"])   # three sub-batches
    det.detect_host(frames)
    got = det.board_poses()
    assert got.shape == (n,) and got.tobytes() == want.tobytes()


def test_board_poses_to_device(oa, scene):
    import torch
    n = 8
    det = detector(oa, scene["tpls"], scene["cam"], n, scene["board"])
    d = device_frames(scene["frames"][:n])
    out = torch.zeros((n, oa.BOARD_DTYPE.itemsize), dtype=torch.uint8, device="cuda:0")
    det.enqueue_device(d.data_ptr(), W_, H_, n)
    det.board_poses_to_device(out.data_ptr())
    det.collect()
    host = det.board_poses()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == host.tobytes() and (host["status"] == 1).all()


def test_setter_refusals(oa, scene):
    lib = oa.hip_lib()
    det = detector(oa, scene["tpls"], scene["cam"], 2)
    ctx = det._ctx

    def set_raw(entries, n=None):
        arr = BC.entries(entries)
        return lib.ocvar_hip_set_board(ctx, arr, len(entries) if n is None else n)

    sq = [[0, 0], [1, 0], [1, 1], [0, 1]]
    assert set_raw([(0, sq)], n=-1) == -2 and set_raw([(0, sq)], n=257) == -2
    assert set_raw([(4096, sq)]) == -2 and set_raw([(1, sq), (1, sq)]) == -2
    assert set_raw([(0, [[0, 0], [1, 0], [0, 1], [1, 1]])]) == -2 and set_raw([(0, [[0, 0], [1, 0], [1, float("nan")], [0, 1]])]) == -2
    d = device_frames(scene["frames"][:2])
    det.enqueue_device(d.data_ptr(), W_, H_, 2)
    assert set_raw(scene["board"]) == -2   # a batch in flight
    assert lib.ocvar_hip_board_poses_to_device(ctx, C.c_void_p(d.data_ptr()), None) == -2   # that batch has no board
    det.collect()
    assert set_raw(scene["board"]) == 0
    det.detect_device(d.data_ptr(), W_, H_, 2)
    assert (det.board_poses()["status"] == 1).all()
    out = (BC.BoardPose * 3)()
    assert lib.ocvar_hip_board_poses(ctx, out, 3) == -2   # more frames than the batch had
    assert set_raw([]) == 0

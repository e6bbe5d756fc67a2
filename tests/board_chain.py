"""Planar marker boards for the board pose tests (ocvar_hip_set_board): the host build of opencv-ar_amd/csrc/board_core.h
(tests/emul/board_emul.cpp), boards rendered at a known pose with ocvar_synth_draw_quads, and the host chain the device must
match -- the oracle's registration, the host refine core on each record, the host board core on the grey image.  Shared by
tests/test_board_cpu.py and tests/test_gpu_board.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import dense_synth as DS
import helpers as H
import refine_chain as RC
from helpers import P
from hostbuild import host_core


class BoardMarker(C.Structure):
    _fields_ = [("templateId", C.c_int), ("pad", C.c_int), ("corner", C.c_double * 8)]


class BoardPose(C.Structure):
    _fields_ = [("glMatrix", C.c_double * 16), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("rms", C.c_double),
                ("n_markers", C.c_int), ("status", C.c_int)]


assert C.sizeof(BoardMarker) == 72 and C.sizeof(BoardPose) == 192


def build_emul():
    L = host_core("board_emul")
    L.board_first_bad_emul.argtypes = [C.c_void_p, C.c_int]
    L.board_solve_obs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.board_solve_obs.restype = None
    L.board_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.board_frame.restype = None
    return L


_synth = None


def synth():
    """the synthetic generator, rebuilt first (a library built before ocvar_synth_draw_quads existed lacks it)"""
    global _synth
    if _synth is None:
        subprocess.check_call(["make", "-C", H.PKG, "lib/libocvar_synth.so"], stdout=subprocess.DEVNULL)
        lib = C.CDLL(os.path.join(H.PKG, "lib", "libocvar_synth.so"))
        lib.ocvar_synth_draw_quads.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int]
        _synth = lib
    return _synth


def entries(board):
    """[(template_id, 4x2 corners)] -> ctypes array of BoardMarker"""
    arr = (BoardMarker * max(len(board), 1))()
    for i, (t, c) in enumerate(board):
        arr[i].templateId = int(t)
        arr[i].corner[:] = [float(v) for v in np.asarray(c, np.float64).reshape(8)]
    return arr


def grid_board(template_ids, cols, rows, length, separation):
    """the layout of opencv_ar_amd.grid_board, restated: marker k at column k % cols, row k // cols"""
    out = []
    for k, t in enumerate(template_ids[:cols * rows]):
        x0, y0 = (k % cols) * (length + separation), (k // cols) * (length + separation)
        out.append((t, np.array([[x0, y0], [x0 + length, y0], [x0 + length, y0 + length], [x0, y0 + length]], np.float64)))
    return out


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def rvec_of(R):
    th = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))
    if th < 1e-12:
        return np.zeros(3)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v * th / (2 * math.sin(th))


def project(K, dist, R, t, pts):
    """pixel projections [n, 2] of board points pts [n, 2] (z = 0), OpenCV's camera model (k1 k2 p1 p2 k3)"""
    P3 = np.c_[pts, np.zeros(len(pts))] @ R.T + t
    x, y = P3[:, 0] / P3[:, 2], P3[:, 1] / P3[:, 2]
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    cd = 1 + (k1 + (k2 + k3 * r2) * r2) * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.c_[xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]]


def cam_arrays(cam):
    K = np.array(cam.cameraMatrix).reshape(3, 3)
    return K, np.array(cam.distCoeffs)


def random_pose(rng, board, fx, size_px, quadrant, tilt_deg, width, height):
    """a pose that shows the board's markers about size_px wide, rotated in plane by quadrant * 90 +- 20 degrees and tilted by
    tilt_deg about a random in-plane axis, its centre near the image centre"""
    gamma = math.radians(90 * quadrant + rng.uniform(-20, 20))
    Rz = np.array([[math.cos(gamma), -math.sin(gamma), 0], [math.sin(gamma), math.cos(gamma), 0], [0, 0, 1]])
    phi = rng.uniform(0, 2 * math.pi)
    Rt = rodrigues(np.array([math.cos(phi), math.sin(phi), 0]) * math.radians(tilt_deg))
    R = Rt @ Rz
    L = np.linalg.norm(board[0][1][1] - board[0][1][0])
    Z = fx * L / size_px
    centre = np.mean(np.concatenate([c for _, c in board]), axis=0)
    t = np.array([rng.uniform(-0.08, 0.08) * width / fx * Z, rng.uniform(-0.08, 0.08) * height / fx * Z, Z]) - R @ np.r_[centre, 0]
    return R, t


def render(board, names, cam, R, t, width=1920, height=1080, background=220):
    """bgr frame of the board at pose (R, t) and the truth image corners [n, 4, 2] (pixel centres at integers)"""
    K, dist = cam_arrays(cam)
    tp = H.template_pixels()
    arrs = [np.ascontiguousarray(tp[n][0]) for n in names]
    st = (H.SynthTemplate * len(arrs))()
    for i, a in enumerate(arrs):
        st[i].pixels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        st[i].h, st[i].w = a.shape
    truth = np.stack([project(K, dist, R, t, c) for _, c in board])
    quads = np.ascontiguousarray((truth + 0.5).reshape(-1, 8))   # (the generator's pixel (x, y) covers [x, x + 1))
    tidx = np.ascontiguousarray([tid for tid, _ in board], np.int32)
    bgr = np.full((height, width, 3), background, np.uint8)
    n = synth().ocvar_synth_draw_quads(P(bgr), width, height, width * 3, st, len(arrs), P(tidx), P(quads), len(board))
    assert n == len(board)
    return bgr, truth


def scenes(n, seed=11, size_range=(90, 160), tilt_max=50, cols=4, rows=3, n_templates=12, cam=None):
    """n boards covering the four in-plane quadrants and tilts 0 .. tilt_max, rendered through camera cam (default
    oracle_camera(1920, 1080)): (names, board, [(bgr, truth, R, t)])"""
    names = DS.library(n_templates, size=4, seed=23)
    board = grid_board(list(range(n_templates)), cols, rows, 1.0, 0.5)
    cam = cam if cam is not None else H.oracle_camera(1920, 1080)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        size = size_range[0] + (size_range[1] - size_range[0]) * ((i * 7) % n) / max(n - 1, 1)
        tilt = tilt_max * ((i * 5) % n) / max(n - 1, 1)
        R, t = random_pose(rng, board, cam.cameraMatrix[0], size, i % 4, tilt, 1920, 1080)
        bgr, truth = render(board, names, cam, R, t)
        out.append((bgr, truth, R, t))
    return names, board, out


def marker_array(records):
    arr = (H.Marker * max(len(records), 1))()
    for i, r in enumerate(records):
        arr[i] = r
    return arr


def host_board(L, gray, records, board, tpls, cam):
    """the host core on one frame: (BoardPose, first [nb], rot [nb])"""
    g = np.ascontiguousarray(gray, np.uint8)
    ent = entries(board)
    out = BoardPose()
    first = np.zeros(max(len(board), 1), np.int32)
    rot = np.zeros(max(len(board), 1), np.int32)
    recs = marker_array(records)
    L.board_frame(P(g), g.shape[1], g.shape[0], g.shape[1], recs, len(records), ent, len(board), tpls, len(tpls), C.byref(cam),
                  C.byref(out), P(first), P(rot))
    return out, first[:len(board)], rot[:len(board)]


def expected(Lr, Lb, bgr, board, tpls, cam, refine=None, prev=None):
    """(records, grey, BoardPose, first, rot) of one frame by the host chain; refine: (w, max_iter, eps) or None"""
    ref, _, img = H.oracle_registration(bgr, tpls, cam, prev=prev)
    gray = np.ascontiguousarray(img[:, :, 0])
    if refine:
        ref = RC.refined_markers(Lr, ref, gray, cam, refine)
    pose, first, rot = host_board(Lb, gray, ref, board, tpls, cam)
    return ref, gray, pose, first, rot


def truth_shift(square, truth_quad):
    """the k with record corner (c + k) & 3 nearest truth corner c, and the largest corner distance under it"""
    s = np.asarray(square, np.float64).reshape(4, 2)
    best = None
    for k in range(4):
        d = np.hypot(*(s[[(c + k) & 3 for c in range(4)]] - truth_quad).T).max()
        if best is None or d < best[1]:
            best = (k, d)
    return best


def pose_errors(pose, R, t):
    """(rotation error in degrees, translation error relative to the distance) of a solved pose against the truth"""
    return rt_errors(rodrigues(np.array(pose.rvec)), np.array(pose.tvec), R, t)


def rt_errors(Rs, ts, R, t):
    """pose_errors of a solved rotation matrix and translation"""
    dR = Rs @ R.T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))
    return ang, np.linalg.norm(ts - t) / np.linalg.norm(t)

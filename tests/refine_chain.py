"""The expected results of corner refinement (ocvar_hip_set_corner_refine) on the CPU: the oracle's unrefined registration, the
host build of opencv-ar_amd/csrc/refine_core.h (tests/emul/refine_emul.cpp) on every output square, and the oracle's pose of the
refined square.  Shared by tests/test_corner_refine_cpu.py and tests/test_gpu_corner_refine.py."""
import ctypes as C

import numpy as np

import helpers as H
from helpers import P
from hostbuild import host_core


def build_emul():
    L = host_core("refine_emul")
    L.refine_weights.argtypes = [C.c_int, C.c_void_p]
    L.refine_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]
    L.refine_points.restype = None
    return L


def refine_points(L, gray, xy, w, max_iter, eps):
    """the host core on corners xy [n, 2] of a grey image: float32 [n, 2]"""
    g = np.ascontiguousarray(gray, np.uint8)
    pts = np.ascontiguousarray(np.asarray(xy, np.float32).reshape(-1, 2)).copy()
    L.refine_points(P(g), g.shape[1], g.shape[0], g.shape[1], P(pts), len(pts), w, max_iter, float(np.float32(eps)))
    return pts


def refined_markers(L, markers, gray, cam, setting):
    """copies of the oracle's marker records with their squares refined on `gray` and their poses solved from those"""
    w, it, eps = setting
    out = []
    for r in markers:
        m = H.Marker.from_buffer_copy(bytes(r))
        sq = refine_points(L, gray, np.array(m.square, np.float32), w, it, eps).reshape(8)
        m.square[:] = [float(v) for v in sq]
        sq = np.ascontiguousarray(np.array(m.square, np.float32))
        gl = np.zeros(16, np.float64)
        H.oracle().orc_square_to_matrix(P(sq), C.byref(cam), C.c_double(m.aspectRatio), P(gl))
        m.glMatrix[:] = gl.tolist()
        out.append(m)
    return out


def expected(L, bgr, tpls, cam, setting, prev=None):
    """(refined marker records, the grey image) of one frame; prev: the previous step's (refined) records"""
    ref, _, img = H.oracle_registration(bgr, tpls, cam, prev=prev)
    gray = np.ascontiguousarray(img[:, :, 0])
    return refined_markers(L, ref, gray, cam, setting), gray


def moved_prev(refined, unrefined, dist=19.99, min_offset=0.05):
    """prev lists that sit at the 20-px tracking boundary (opencvar.cpp's cvarTrack: all four corners closer than 20 px).  Each
    marker whose refinement moved a corner by at least min_offset px is moved by `dist` px along its largest corner offset e:
    the refined record then has that corner |e| + dist >= 20 px from this frame's (unrefined) square, so it is not tracked,
    while the unrefined record moved the same way has every corner dist < 20 px from it, so it is.  Returns (refined prev,
    unrefined prev)."""
    pr, pu = [], []
    for e, r in zip(refined, unrefined):
        E = np.array(e.square, np.float64).reshape(4, 2)
        U = np.array(r.square, np.float64).reshape(4, 2)
        off = np.hypot(*(E - U).T)
        j = int(np.argmax(off))
        if off[j] < min_offset:
            continue
        d = dist * (E[j] - U[j]) / off[j]
        for src, base, out in ((e, E, pr), (r, U, pu)):
            m = H.Marker.from_buffer_copy(bytes(src))
            m.square[:] = [float(v) for v in np.float32(base + d).reshape(8)]
            out.append(m)
    return pr, pu


def records_differ(a, b):
    return len(a) != len(b) or any(bytes(x) != bytes(y) for x, y in zip(a, b))


POSE_RTOL = 1e-4


def check(markers, counts, f, exp, where=""):
    """row f of a device result against the expected records: ids, templates, scores bit-exact, squares bit-exact, poses within
    the pose bar"""
    assert counts[f] == len(exp), ("count", where, f, int(counts[f]), len(exp))
    for k, r in enumerate(exp[:markers.shape[1]]):
        m = markers[f, k]
        assert m["templateId"] == r.templateId and m["markerId"] == r.markerId and m["score"] == r.score, ("ids", where, f, k)
        assert np.array_equal(m["square"], np.array(r.square, np.float32)), (
            "square", where, f, k, m["square"].tolist(), list(r.square))
        g = np.array(r.glMatrix)
        assert np.abs(m["glMatrix"] - g).max() <= POSE_RTOL * max(1.0, np.abs(g).max()), ("pose", where, f, k)


def corner_errors(squares, truth):
    """per-corner distances of detected squares ([n, 8], pixel centres at integers) to the nearest truth quad (corners at
    +0.5), under the best cyclic shift of the corners; squares with no truth quad within 10 px are left out"""
    quads = [t["corner"] for t in truth]
    errs = []
    for s in squares:
        c = np.asarray(s, np.float64).reshape(4, 2) + 0.5
        best = None
        for q in quads:
            for sh in range(4):
                d = np.hypot(*(c - np.roll(q, -sh, axis=0)).T)
                if best is None or d.max() < best.max():
                    best = d
        if best is not None and best.max() < 10:
            errs.extend(best.tolist())
    return np.array(errs)

"""CPU tests of sub-pixel corner refinement (ocvar_hip_set_corner_refine): the host build of opencv-ar_amd/csrc/refine_core.h
against a plain restatement of its equations, its accuracy on rendered corners and on the synthetic frames, the Python argument
checks, and the new entry points of the three libraries."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import refine_chain as RC


@pytest.fixture(scope="module")
def L():
    return RC.build_emul()


def restated(gray, c0, w, max_iter, eps):
    """The refinement's steps 1-6 as written (include/ocvar_hip.h, refine_core.h), in numpy, one point at a time."""
    Hh, Ww = gray.shape
    img = gray.astype(np.float32)
    g = np.array([np.float32(np.exp(-(k * k) / (w * w))) for k in range(-w, w + 1)], np.float32)
    cx, cy = np.float32(c0[0]), np.float32(c0[1])
    for _ in range(max_iter):
        ox, oy = cx - np.float32(w + 1), cy - np.float32(w + 1)
        fx, fy = np.floor(ox), np.floor(oy)
        ax, ay = np.float32(ox - fx), np.float32(oy - fy)
        side = 2 * w + 3
        Pt = np.zeros((side, side), np.float32)
        for pj in range(side):
            for pi in range(side):
                xa, ya = int(fx) + pi, int(fy) + pj
                x0, x1 = min(max(xa, 0), Ww - 1), min(max(xa + 1, 0), Ww - 1)
                y0, y1 = min(max(ya, 0), Hh - 1), min(max(ya + 1, 0), Hh - 1)
                Pt[pj, pi] = (img[y0, x0] * (1 - ax) * (1 - ay) + img[y0, x1] * ax * (1 - ay) + img[y1, x0] * (1 - ax) * ay
                              + img[y1, x1] * ax * ay)
        a = b = c = b1 = b2 = 0.0
        for j in range(-w, w + 1):
            for i in range(-w, w + 1):
                pi, pj = i + w + 1, j + w + 1
                gx = float(Pt[pj, pi + 1] - Pt[pj, pi - 1])
                gy = float(Pt[pj + 1, pi] - Pt[pj - 1, pi])
                m = float(g[i + w] * g[j + w])
                a += m * gx * gx
                b += m * gx * gy
                c += m * gy * gy
                b1 += m * (gx * gx * i + gx * gy * j)
                b2 += m * (gx * gy * i + gy * gy * j)
        det = a * c - b * b
        if abs(det) <= np.finfo(np.float64).eps ** 2:
            break
        nx = np.float32(float(cx) + (c * b1 - b * b2) / det)   # the step in double, the new corner rounded to float
        ny = np.float32(float(cy) + (a * b2 - b * b1) / det)
        err = float((nx - cx) ** 2 + (ny - cy) ** 2)
        cx, cy = nx, ny
        if cx < 0 or cx >= Ww or cy < 0 or cy >= Hh or err <= np.float32(eps) ** 2:
            break
    if abs(cx - np.float32(c0[0])) > w or abs(cy - np.float32(c0[1])) > w:
        return np.float32(c0[0]), np.float32(c0[1])
    return cx, cy


def render(W, H_, cx, cy, theta, kind="L", lo=40, hi=210, ss=16):
    """a corner at (cx, cy) (pixel centres at integer coordinates), 16x16 supersampled: kind "L" one quadrant bright (the corner
    of a marker), "X" two opposite quadrants (a checkerboard corner); edges at angle theta"""
    o = (np.arange(ss) + 0.5) / ss - 0.5
    ys, xs = np.mgrid[0:H_, 0:W]
    dx = xs[:, :, None, None] + o[None, None, None, :] - cx
    dy = ys[:, :, None, None] + o[None, None, :, None] - cy
    u = np.cos(theta) * dx + np.sin(theta) * dy
    v = -np.sin(theta) * dx + np.cos(theta) * dy
    inside = (u > 0) & (v > 0) if kind == "L" else (u > 0) == (v > 0)
    return np.round(lo + (hi - lo) * inside.mean(axis=(2, 3))).astype(np.uint8)


def scene(W=96, H_=80, seed=0):
    """rendered L corners at random angles plus noise: a busy grey image for the restatement"""
    rng = np.random.default_rng(seed)
    img = np.zeros((H_, W), np.float64)
    pts = []
    for _ in range(6):
        cx, cy = rng.uniform(2, W - 3), rng.uniform(2, H_ - 3)
        img += render(W, H_, cx, cy, rng.uniform(0, 2 * np.pi), lo=0, hi=60, ss=4)
        pts.append((cx, cy))
    img += rng.normal(0, 3, img.shape)
    return np.clip(img + 30, 0, 255).astype(np.uint8), pts


def agree(L, gray, starts, w, max_iter, eps):
    got = RC.refine_points(L, gray, np.array(starts, np.float32), w, max_iter, eps)
    for k, s in enumerate(starts):
        want = restated(gray, np.array(s, np.float32), w, max_iter, eps)
        assert np.abs(got[k] - np.array(want, np.float32)).max() <= 1e-3, (w, s, got[k].tolist(), [float(v) for v in want])
    return got


@pytest.mark.parametrize("w", [1, 5, 15])
def test_core_matches_the_restated_equations(L, w):
    gray, pts = scene(seed=w)
    starts = [(round(x) + dx, round(y) + dy) for x, y in pts for dx, dy in ((0, 0), (1, -1))]
    agree(L, gray, starts, w, 30, 0.1)
    agree(L, gray, starts[:4], w, 12, 0.0)   # eps = 0: only max_iter (or det / the frame) stops


@pytest.mark.parametrize("w", [1, 5, 15])
def test_core_at_the_frame_edges(L, w):
    """corners within w + 1 px of every edge: the patch reaches past the frame (replicate border)"""
    Wd, Hd = 64, 48
    rng = np.random.default_rng(10 + w)
    for cx, cy in ((0.7, 20.2), (Wd - 1.4, 20.6), (30.3, 0.6), (30.8, Hd - 1.3), (1.2, 1.1), (Wd - 1.6, Hd - 1.6)):
        img = render(Wd, Hd, cx, cy, rng.uniform(0, 2 * np.pi), kind="X")
        starts = [(min(max(round(cx) + dx, 0), Wd - 1), min(max(round(cy) + dy, 0), Hd - 1)) for dx in (-1, 0, 1) for dy in (-w - 1, 0, w)]
        starts = [(x, min(max(y, 0), Hd - 1)) for x, y in starts]
        agree(L, img, starts, w, 30, 0.05)


def test_flat_patch_stops_at_once(L):
    """no gradient: det = 0, the corner stays where it started"""
    for w in (1, 5, 15):
        flat = np.full((40, 50), 128, np.uint8)
        got = agree(L, flat, [(10.0, 10.0), (25.5, 19.25)], w, 30, 0.1)
        assert got.tolist() == [[10.0, 10.0], [25.5, 19.25]]
        edge = np.zeros((40, 50), np.uint8)   # a straight edge: gradients in one direction only, det = 0 as well
        edge[:, 25:] = 200
        got = agree(L, edge, [(25.0, 20.0)], w, 30, 0.1)
        assert got.tolist() == [[25.0, 20.0]]


def test_far_start_keeps_its_corner(L):
    """a start that converges more than w px away keeps c0"""
    img = render(80, 80, 40.3, 40.6, 0.4, kind="X")
    start = (46.0, 42.0)
    free = RC.refine_points(L, img, np.array(start, np.float32), 15, 30, 0.01)[0]
    assert abs(free[0] - 40.3) < 0.2 and abs(free[1] - 40.6) < 0.2   # the corner a wider window finds, 5.7 px off in x
    got = agree(L, img, [start], 5, 30, 0.01)
    assert got[0].tolist() == list(start)


def test_weights_are_the_gaussian_of_the_spec(L):
    for w in (1, 5, 15):
        g = np.zeros(2 * w + 1, np.float32)
        L.refine_weights(w, g.ctypes.data)
        want = np.array([np.float32(np.exp(-(k * k) / (w * w))) for k in range(-w, w + 1)], np.float32)
        assert np.abs(g - want).max() <= 1e-7 and g[w] == 1.0


# Rendered corners, 16x16 supersampled at random sub-pixel positions and angles, started up to 2 px off (w = 5, 30 steps,
# eps 0.01).  Measured over these 48 cases each: a checkerboard corner ("X") lands within 0.11 px of the truth (median 0.04); a
# marker's corner ("L", one bright quadrant) within 0.37 px (median 0.19) -- cornerSubPix's own bias on a convex corner, where
# the gradients next to the apex point along the diagonal.  The starts were 0.6 .. 3.4 px off (median 2.1).
IDEAL_TOL = {"X": 0.16, "L": 0.5}


@pytest.mark.parametrize("kind", ["X", "L"])
def test_accuracy_on_rendered_corners(L, kind):
    rng = np.random.default_rng(3)
    errs, start_errs = [], []
    for _ in range(48):
        cx, cy = 32 + rng.uniform(-0.5, 0.5), 32 + rng.uniform(-0.5, 0.5)
        img = render(64, 64, cx, cy, rng.uniform(0, 2 * np.pi), kind=kind)
        st = np.array([round(cx) + rng.integers(-2, 3), round(cy) + rng.integers(-2, 3)], np.float32)
        r = RC.refine_points(L, img, st, 5, 30, 0.01)[0]
        errs.append(np.hypot(r[0] - cx, r[1] - cy))
        start_errs.append(np.hypot(st[0] - cx, st[1] - cy))
    errs = np.array(errs)
    assert errs.max() <= IDEAL_TOL[kind], (kind, float(np.median(errs)), float(errs.max()))
    assert np.median(errs) < 0.25 * np.median(start_errs)


# synth_config(3) frames 0..23 (1080p, 16 markers of 3 templates each; the registration keeps one marker per template), corner
# errors against the generator's truth (corner + 0.5 against the truth's pixel-centre convention, best cyclic shift), 232 corners.
# Measured: unrefined median 0.60 px, 95th percentile 1.49 px; refined (5 / 30 / 0.1) median 0.21 px, 95th percentile 0.38 px
# (at w = 15: 0.38 / 0.69 px -- the window then reaches the code cells).
SYNTH_FRAMES = 24
SYNTH_LIMITS = {"median": 0.3, "p95": 0.5}


def test_accuracy_on_synthetic_frames(L):
    cfg = H.synth_config(3)
    tpls, cam = H.oracle_templates(), H.oracle_camera(cfg.width, cfg.height)
    e0, e1 = [], []
    for f in range(SYNTH_FRAMES):
        bgr, truth = H.synth_frame(cfg, f)
        ref, _, img = H.oracle_registration(bgr, tpls, cam)
        gray = np.ascontiguousarray(img[:, :, 0])
        sq0 = [np.array(r.square, np.float32) for r in ref]
        sq1 = [RC.refine_points(L, gray, s, 5, 30, 0.1).reshape(8) for s in sq0]
        e0.append(RC.corner_errors(sq0, truth))
        e1.append(RC.corner_errors(sq1, truth))
    e0, e1 = np.concatenate(e0), np.concatenate(e1)
    assert len(e0) == len(e1) >= 100
    m0, p0, m1, p1 = np.median(e0), np.percentile(e0, 95), np.median(e1), np.percentile(e1, 95)
    assert m1 <= SYNTH_LIMITS["median"] and p1 <= SYNTH_LIMITS["p95"], (m0, p0, m1, p1)
    assert m1 < 0.5 * m0 and p1 < 0.5 * p0, (m0, p0, m1, p1)


def test_python_argument_checks():
    import opencv_ar_amd as oa
    assert oa.corner_refine_args(5, 30, 0.1) == (5, 30, 0.1)
    assert oa.corner_refine_args(0, 1, 0) == (0, 1, 0.0)
    assert oa.corner_refine_args(15, 100, 2) == (15, 100, 2.0)
    for bad in ((-1, 30, 0.1), (16, 30, 0.1), (5, 0, 0.1), (5, 101, 0.1), (5, 30, -0.01), (5, 30, float("nan")),
                (5.0, 30, 0.1), (True, 30, 0.1), (5, "30", 0.1), (5, 30, None)):
        with pytest.raises(ValueError):
            oa.corner_refine_args(*bad)
    for cls in (oa.Detector, oa.Pipe):
        assert callable(getattr(cls, "set_corner_refine"))


def test_setters_reject_bad_arguments_before_any_device_call():
    import opencv_ar_amd as oa
    lib = oa.hip_lib()
    assert lib.ocvar_hip_set_corner_refine(None, 5, 30, 0.1) == -2
    assert lib.ocvar_hip_pipe_set_corner_refine(None, 5, 30, 0.1) == -2


def test_new_symbols_load():
    import opencv_ar_amd as oa
    assert hasattr(oa.hip_lib(), "ocvar_hip_set_corner_refine") and hasattr(oa.hip_lib(), "ocvar_hip_pipe_set_corner_refine")
    assert "ocvar_hip_set_corner_refine" in oa.HIP_SYMBOLS and "ocvar_hip_pipe_set_corner_refine" in oa.HIP_SYMBOLS
    multi = C.CDLL(os.path.join(oa.LIB_DIR, "libocvar_multi.so"))
    assert hasattr(multi, "ocvar_multi_set_corner_refine")
    host = C.CDLL(oa.HOST_LIB)
    assert hasattr(host, "cvarSetCornerRefine")


def test_tracking_boundary_case_tells_refined_from_unrefined_prev(L):
    """the prev lists of the GPU tracking-boundary test: with the refined records as prev the markers are not tracked, with the
    unrefined ones moved the same way they are, so the two chains differ"""
    cfg = H.synth_config(3)
    tpls, cam = H.oracle_templates(), H.oracle_camera(cfg.width, cfg.height)
    for f in range(2):
        bgr = H.synth_frame(cfg, f)[0]
        ref, _, img = H.oracle_registration(bgr, tpls, cam)
        refined = RC.refined_markers(L, ref, np.ascontiguousarray(img[:, :, 0]), cam, (5, 30, 0.1))
        pr, pu = RC.moved_prev(refined, ref)
        assert pr and len(pr) == len(pu)
        er, _ = RC.expected(L, bgr, tpls, cam, (5, 30, 0.1), prev=pr)
        eu, _ = RC.expected(L, bgr, tpls, cam, (5, 30, 0.1), prev=pu)
        assert len(er) == len(ref) and len(eu) > len(ref) and RC.records_differ(er, eu)   # none tracked / tracked ones kept

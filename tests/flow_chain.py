"""Flow tracking for the flow tests (ocvar_hip_flow_records): the host build of opencv-ar_amd/csrc/flow_core.h
(tests/emul/flow_emul.cpp), a plain numpy float64 restatement of the equations -- written from the text of the definition
(include/ocvar_hip.h and the head of flow_core.h), not from the code: the independent yardstick --, textured frames, exact shifts
and rendered view pairs.  Frames, records and guard bytes are frame_kit's.  Shared by tests/test_flow_cpu.py and
tests/test_gpu_flow.py.

The oracle has no pyrDown entry point of its own (orc_binarise returns only the threshold and the pyrUp of its pyrDown), so the
pyramid is compared against the numpy restatement here."""
import ctypes as C
import math

import numpy as np

import helpers as H
import persp_synth as PS
from frame_kit import FORMATS, GUARD, records
from helpers import P
from hostbuild import host_core

POSE = 1
DEFAULTS = dict(half_win=10, levels=3, max_iter=30, flags=0, eps=0.03, min_eig=1e-3, max_err=0.0, fb_max=0.0)


class FlowParams(C.Structure):  # OcvarFlowParams
    _fields_ = [("half_win", C.c_int), ("levels", C.c_int), ("max_iter", C.c_int), ("flags", C.c_int),
                ("eps", C.c_float), ("min_eig", C.c_float), ("max_err", C.c_float), ("fb_max", C.c_float)]


assert C.sizeof(FlowParams) == 32


def params(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return FlowParams(**d)


def build_emul():
    L = host_core("flow_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.flow_geom_emul.argtypes = [i, i, i, i, vp, vp]
    L.flow_grey_level_emul.argtypes = [vp, i, i, ll, i, vp, i]
    L.flow_pyramid_level_emul.argtypes = [vp, i, i, i, vp, i]
    L.flow_build_pyramid_emul.argtypes = [vp, i, i, ll, i, i, i, vp]
    L.flow_track_frame_emul.argtypes = [vp, ll, vp, ll, i, i, i, vp, vp, vp, i, i, vp, vp, vp]
    L.flow_track_points_emul.argtypes = [vp, vp, i, i, vp, vp, i, vp, vp, vp]
    return L


# ---- the host build ------------------------------------------------------------------------------------------------------------------

def host_geom(L, W, Hh, half_win, levels):
    """(L, [(w, h, pitch, off)] of the six levels, bytes)"""
    dims, offs = np.zeros(19, np.int32), np.zeros(7, np.int64)
    L.flow_geom_emul(W, Hh, half_win, levels, P(dims), P(offs))
    return int(dims[0]), [(int(dims[1 + l]), int(dims[7 + l]), int(dims[13 + l]), int(offs[l])) for l in range(6)], int(offs[6])


def host_level_up(L, img):
    """the level above the grey image img"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    L.flow_pyramid_level_emul(P(img), w, h, w, P(out), out.shape[1])
    return out


def host_points(L, A, B, pts, p):
    """the host core on points pts [n, 2] from grey image A to B -> (out [n, 2] float32, codes [n], err [n])"""
    A, B = np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.uint8)
    assert A.shape == B.shape and A.ndim == 2
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out, codes, err = np.zeros_like(pts), np.zeros(len(pts), np.int32), np.zeros(len(pts), np.float32)
    L.flow_track_points_emul(P(A), P(B), A.shape[1], A.shape[0], C.byref(p), P(pts), len(pts), P(out), P(codes), P(err))
    return out, codes, err


def host_flow(L, prev, nxt, recs, counts, p, cam=None, out=None, per_frame=None, prev_buf=None, next_buf=None):
    """the host core on the frame blocks prev and nxt (Frames; *_buf: other buffers of their layout) under recs [n, slots] and counts
    -> (records, status [n, slots], err [n, slots, 4]); `out`: the block the records are written into (default: a copy of recs),
    status and err start as guard bytes where the device leaves them untouched"""
    recs = np.ascontiguousarray(recs)
    n, slots = recs.shape
    assert per_frame in (None, slots) and prev.n == nxt.n == n
    res = (recs if out is None else out).copy()
    status = np.zeros((n, slots), np.int32)
    err = np.frombuffer(np.full(n * slots * 16, GUARD, np.uint8).tobytes(), np.float32).reshape(n, slots, 4).copy()
    cam = H.Camera() if cam is None else cam
    pb = prev.buf if prev_buf is None else prev_buf
    nb = nxt.buf if next_buf is None else next_buf
    for f in range(n):
        src = recs[f].copy()
        L.flow_track_frame_emul(pb.ctypes.data + prev.offset(f), prev.row_stride, nb.ctypes.data + nxt.offset(f), nxt.row_stride,
                                prev.width, prev.height, prev.fmt, C.byref(p), C.byref(cam), src.ctypes.data, int(counts[f]), slots,
                                res[f].ctypes.data, status[f].ctypes.data, err[f].ctypes.data)
    return res, status, err


# ---- the numpy restatement (float64) ---------------------------------------------------------------------------------------------------

def np_grey(frame, fmt):
    """level 0 of a frame [H, W] or [H, W, bpp] in format fmt"""
    fmt = FORMATS[fmt] if isinstance(fmt, str) else fmt
    f = np.asarray(frame).astype(np.int64)
    if fmt == 4:
        return f.reshape(f.shape[0], f.shape[1]).astype(np.uint8)
    b, r = (f[..., 0], f[..., 2]) if fmt in (0, 2) else (f[..., 2], f[..., 0])
    return ((1868 * b + 9617 * f[..., 1] + 4899 * r + 8192) >> 14).astype(np.uint8)


def np_level_up(img):
    """pyrDown of an 8-bit image: 1 4 6 4 1 both ways, reflection without the edge pixel, (sum + 128) >> 8"""
    h, w = img.shape
    p = np.pad(img.astype(np.int64), 2, mode="reflect")
    k = (1, 4, 6, 4, 1)
    w2, h2 = (w + 1) // 2, (h + 1) // 2
    hor = sum(k[i] * p[:, i:i + 2 * w2:2][:, :w2] for i in range(5))
    ver = sum(k[j] * hor[j:j + 2 * h2:2][:h2] for j in range(5))
    return ((ver + 128) >> 8).astype(np.uint8)


def np_pyramid(img, half_win, levels):
    pyr = [np.asarray(img, np.uint8)]
    while len(pyr) <= levels:
        nxt = np_level_up(pyr[-1])
        if min(nxt.shape) < 2 * half_win + 3:
            break
        pyr.append(nxt)
    return pyr


def np_sample(img, cx, cy, w):
    """the (2w+3)^2 patch around (cx, cy): bilinear, coordinates clamped to the image"""
    h, wd = img.shape
    side = 2 * w + 3
    ox, oy = cx - (w + 1), cy - (w + 1)
    fx, fy = math.floor(ox), math.floor(oy)
    ax, ay = ox - fx, oy - fy
    xs, ys = fx + np.arange(side), fy + np.arange(side)
    xa, xb = np.clip(xs, 0, wd - 1), np.clip(xs + 1, 0, wd - 1)
    ya, yb = np.clip(ys, 0, h - 1), np.clip(ys + 1, 0, h - 1)
    f = img.astype(np.float64)
    top = f[np.ix_(ya, xa)] * (1 - ax) + f[np.ix_(ya, xb)] * ax
    bot = f[np.ix_(yb, xa)] * (1 - ax) + f[np.ix_(yb, xb)] * ax
    return top * (1 - ay) + bot * ay


def np_track_point(pa, pb, p, half_win, max_iter, eps, min_eig, max_err):
    """one corner from pyramid pa to pb -> (code, q, err)"""
    w = half_win
    hh, ww = pa[0].shape
    p = np.asarray(p, np.float64)
    if not (np.isfinite(p).all() and 0 <= p[0] <= ww - 1 and 0 <= p[1] <= hh - 1):
        return -1, p, -1.0
    n = (2 * w + 1) ** 2
    g = np.zeros(2)
    d = np.zeros(2)
    for l in range(len(pa) - 1, -1, -1):
        pl = p / 2.0 ** l
        lh, lw = pa[l].shape
        I = np_sample(pa[l], pl[0], pl[1], w)
        Ic = I[1:-1, 1:-1]
        Ix, Iy = 0.5 * (I[1:-1, 2:] - I[1:-1, :-2]), 0.5 * (I[2:, 1:-1] - I[:-2, 1:-1])
        a, b, c = (Ix * Ix).sum(), (Ix * Iy).sum(), (Iy * Iy).sum()
        T = min_eig * n
        det = a * c - b * b
        texture = a - T >= 0 and c - T >= 0 and (a - T) * (c - T) - b * b >= 0 and abs(det) > np.finfo(np.float64).eps ** 2
        d = np.zeros(2)
        if not texture:
            if l == 0:
                return -2, p, -1.0
        else:
            for _ in range(max_iter):
                pos = pl + g + d
                J = np_sample(pb[l], pos[0], pos[1], w)[1:-1, 1:-1]
                e1, e2 = ((Ic - J) * Ix).sum(), ((Ic - J) * Iy).sum()
                step = np.array([(c * e1 - b * e2) / det, (a * e2 - b * e1) / det])
                new = pl + g + d + step
                if not (0 <= new[0] <= lw - 1 and 0 <= new[1] <= lh - 1):
                    if l == 0:
                        return -3, p, -1.0
                    break
                d = d + step
                if step @ step <= eps * eps:
                    break
        if l > 0:
            g = 2 * (g + d)
    q = p + g + d
    J = np_sample(pb[0], q[0], q[1], w)[1:-1, 1:-1]
    err = float(np.abs(Ic - J).mean())
    if max_err > 0 and err > max_err:
        return -4, q, err
    return 1, q, err


def np_points(A, B, pts, half_win=10, levels=3, max_iter=30, eps=0.03, min_eig=1e-3, max_err=0.0, fb_max=0.0, **_):
    """the restatement on points pts [n, 2] from grey image A to B -> (out [n, 2] float64, codes [n], err [n])"""
    pa, pb = np_pyramid(A, half_win, levels), np_pyramid(B, half_win, levels)
    out, codes, errs = [], [], []
    for p in np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64):
        code, q, err = np_track_point(pa, pb, p, half_win, max_iter, eps, min_eig, max_err)
        if code == 1 and fb_max > 0:
            back, r, _ = np_track_point(pb, pa, q, half_win, max_iter, eps, min_eig, max_err)
            if back != 1 or ((r - p) ** 2).sum() > fb_max ** 2:
                code = -5
        out.append(q), codes.append(code), errs.append(err)
    return np.array(out), np.array(codes), np.array(errs)


def params_dict(p):
    return {k: getattr(p, k) for k, _ in FlowParams._fields_}


# ---- frames ----------------------------------------------------------------------------------------------------------------------------

def texture(rng, width, height, cell=6):
    """a smooth random grey image with texture at every scale the pyramid sees: noise of several cell sizes, summed"""
    img = np.zeros((height, width))
    for c in (cell, 3 * cell, 9 * cell):
        small = rng.uniform(0, 1, (height // c + 3, width // c + 3))
        big = np.kron(small, np.ones((c, c)))[:height, :width]
        img += big
    k = np.array([1, 4, 6, 4, 1]) / 16.0
    for _ in range(2):
        img = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 2, mode="edge"), k, "valid"), 1, img)
        img = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 2, mode="edge"), k, "valid"), 0, img)
    img -= img.min()
    return np.rint(img / img.max() * 255).astype(np.uint8)


def shifted_pair(rng, width, height, dx, dy, cell=6):
    """(A, B) grey images with B(x + dx, y + dy) = A(x, y): both cut out of one larger texture, nothing wraps"""
    m = max(abs(dx), abs(dy)) + 1
    big = texture(rng, width + 2 * m, height + 2 * m, cell)
    return big[m:m + height, m:m + width].copy(), big[m - dy:m - dy + height, m - dx:m - dx + width].copy()


def fill_frames(frames, greys):
    """the grey images greys [n] into the Frames block (all colour channels alike, byte 3 of four-channel pixels left random)"""
    for f, g in enumerate(greys):
        v = frames.view(f)
        for c in range(min(frames.bpp, 3)):
            v[..., c] = g
    return frames


# rendered view pairs: one marker at two poses (u, v, size, tilt, gamma, phi) -> (u', v', ...)
def _moves(width, height):
    u, v, s = 0.45 * width, 0.5 * height, 0.3 * height
    base = (u, v, s, 20.0, 12.0, 40.0)
    return [("shift3", base, (u + 3, v, s, 20.0, 12.0, 40.0)),
            ("shift12", base, (u + 8.5, v - 8.5, s, 20.0, 12.0, 40.0)),
            ("shift40", base, (u + 32, v + 24, s, 20.0, 12.0, 40.0)),
            ("rot5", base, (u, v, s, 20.0, 17.0, 40.0)),
            ("tilt10", base, (u, v, s, 30.0, 12.0, 40.0))]


VIEW_SIZES = [(160, 120), (640, 480)]


def view_pairs():
    """[(name, width, height, cam, frame A (bgr), frame B (bgr), true quad in A [4, 2], true quad in B [4, 2])]"""
    out = []
    for width, height in VIEW_SIZES:
        cam = PS.camera(width, height)
        for name, pa, pb in _moves(width, height):
            fa, ma = PS.render(width, height, cam, [PS.pose(cam, *pa) + (2, pa[3], pa[2], None)])
            fb, mb = PS.render(width, height, cam, [PS.pose(cam, *pb) + (2, pb[3], pb[2], None)])
            out.append(("%s-%d" % (name, width), width, height, cam, fa, fb, np.array(ma[0].quad), np.array(mb[0].quad)))
    return out


# ---- status codes --------------------------------------------------------------------------------------------------------------------

GOOD = [30, 50, 70, 52, 68, 80, 28, 78]   # a convex quad on code_scene's texture


def code_scene():
    """a 128 x 96 texture with a constant region (x 90 .. 127, y 0 .. 40), its shift by (3, 2) and an occluded copy of that"""
    rng = np.random.default_rng(11)
    W, Hh = 128, 96
    A, B = shifted_pair(rng, W, Hh, 3, 2)
    A[0:41, 90:] = 77
    B[0:43, 93:] = 77
    occl = B.copy()
    occl[40:76, 24:60] = texture(np.random.default_rng(12), 36, 36, cell=3)   # over the corner (40, 56) -> (43, 58)
    return dict(W=W, H=Hh, A=A, B=B, occl=occl)


def code_records(W):
    """[1, 6] records on code_scene's A -> B with the statuses 1, -1, -2, -6, -6 and one more for a slot beyond the count"""
    sq = []
    sq.append(GOOD)                                         # 1
    sq.append([30, 50, np.nan, 52, 110, 20, 28, 78])        # corner 1 -1 before corner 2 -2
    sq.append([110, 20, 70, 52, W, 80, 28, 78])             # corner 0 -2 before corner 2 -1
    sq.append([30, 50, 68, 80, 70, 52, 28, 78])             # a bow-tie: every corner tracks, the quad is folded
    sq.append([30, 50, 30, 50, 70, 52, 28, 78])             # two corners alike: they track alike, no strict turn there
    sq.append(GOOD)                                         # beyond the count
    recs = records(sq, template_ids=np.arange(6) + 3).reshape(1, 6)
    recs["glMatrix"] = np.random.default_rng(14).normal(size=(1, 6, 16))
    recs["aspectRatio"] = 1.25
    return recs


# ---- a marker that moves faster than the tracking stage's 20 px ------------------------------------------------------------------------

def moving_marker(n=3, width=320, height=240, step=(24.0, 18.0), size=70.0, template=2):
    """(cam, templates, frames [n, H, W, 3] bgr): one marker of `template`, its centre moving by `step` (30 px) from frame to frame"""
    cam = PS.camera(width, height)
    frames = []
    for t in range(n):
        spec = (90.0 + step[0] * t, 80.0 + step[1] * t, size, 15.0, 10.0, 30.0)
        frames.append(PS.render(width, height, cam, [PS.pose(cam, *spec) + (template, spec[3], spec[2], None)])[0])
    return cam, H.oracle_templates(PS.NAMES), np.stack(frames)

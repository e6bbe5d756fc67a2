"""Undistortion for the undistort tests (ocvar_hip_undistort / ocvar_hip_undistort_records): the host build of
opencv-ar_amd/csrc/undistort_core.h (tests/emul/undistort_emul.cpp), the lenses, guarded destination buffers, and distort_image,
which makes a truly distorted view of a pinhole-rendered frame in numpy.  Frames, records and guard bytes are frame_kit's.
Shared by tests/test_undistort_cpu.py and tests/test_gpu_undistort.py."""
import ctypes as C

import numpy as np

import helpers as H
import persp_synth as PS
from frame_kit import GUARD, LEAD, Frames
from helpers import P
from hostbuild import host_core

# name -> (k1 k2 p1 p2 k3, shift of the principal point in pixels)
LENSES = {
    "BARREL": (list(PS.DIST), (0.0, 0.0)),                              # no destination pixel maps outside the frame
    "PINCUSHION": ([0.21, -0.09, 0.0015, -0.0008, 0.02], (0.0, 0.0)),   # about a ninth of the destination pixels map outside
    "ZERO": ([0.0] * 5, (0.0, 0.0)),
    "OFF_CENTRE": (list(PS.DIST), (37.25, -21.5)),
    "WILD": ([1e6, 0.0, 0.0, 0.0, 0.0], (0.0, 0.0)),                    # coordinates beyond the int range: everything outside
}


def build_emul():
    L = host_core("undistort_emul")
    L.undistort_frame_emul.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
    L.undistort_records_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.undistort_source_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.undistort_point_emul.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.undistort_cam_ok_emul.argtypes = [C.c_void_p]
    return L


def camera(width, height, lens):
    """the default camera scaled to the frame with the named lens (or a list of five coefficients)"""
    dist, (dx, dy) = LENSES[lens] if isinstance(lens, str) else (list(lens), (0.0, 0.0))
    cam = H.oracle_camera(width, height)
    cam.distCoeffs[:] = dist
    cam.cameraMatrix[2] += dx
    cam.cameraMatrix[5] += dy
    return cam


def dst_frames(n, width, height, fmt, row_pad=0, frame_gap=0, lead=LEAD):
    """destination frames: guarded Frames, all GUARD, whose first frame starts `lead` bytes into the buffer (an odd lead: an odd
    address, device allocations being aligned)"""
    return Frames(n, width, height, fmt, row_pad=row_pad, frame_gap=frame_gap, lead=lead, fill=GUARD)


def host_undistort(L, src, cam, dst, buf=None):
    """the host core on the frames of src.buf (or buf) -> dst's buffer, filled"""
    assert (src.n, src.width, src.height, src.fmt) == (dst.n, dst.width, dst.height, dst.fmt)
    sb = src.buf if buf is None else buf
    out = dst.buf.copy()
    for f in range(src.n):
        L.undistort_frame_emul(sb.ctypes.data + src.offset(f), src.width, src.height, src.row_stride, src.fmt, C.byref(cam),
                               out.ctypes.data + dst.offset(f), dst.row_stride)
    return out


def host_undistort_image(L, img, cam):
    """the host core on one contiguous [H, W] or [H, W, bpp] uint8 image (bpp 3: bgr, 4: bgra) -> the undistorted image"""
    img = np.ascontiguousarray(img)
    bpp = 1 if img.ndim == 2 else img.shape[2]
    out = np.zeros_like(img)
    L.undistort_frame_emul(P(img), img.shape[1], img.shape[0], img.shape[1] * bpp, {1: 4, 3: 0, 4: 2}[bpp], C.byref(cam), P(out), img.shape[1] * bpp)
    return out


def host_records(L, cam, recs, counts, per_frame=None):
    """the host core on recs [n, per_frame] records -> a copy with the slots below min(count, per_frame) mapped"""
    recs = np.ascontiguousarray(recs)
    slots = recs.shape[1] if per_frame is None else per_frame
    assert recs.shape[1] == slots
    out = recs.copy()
    for f in range(recs.shape[0]):
        n = L.undistort_records_emul(C.byref(cam), recs[f].ctypes.data, int(counts[f]), slots, out[f].ctypes.data)
        assert n == max(0, min(int(counts[f]), slots))
    return out


def frame_map(L, cam, uv):
    """the frame map's source positions of destination positions uv [n, 2] -> [n, 2] float64"""
    uv = np.ascontiguousarray(uv, np.float64)
    out = np.zeros_like(uv)
    L.undistort_source_emul(C.byref(cam), P(uv), len(uv), P(out))
    return out


def record_map(L, cam, uv):
    """the record map of points uv [n, 2], before its rounding to float32 -> [n, 2] float64"""
    uv = np.ascontiguousarray(uv, np.float64)
    out = np.zeros_like(uv)
    L.undistort_point_emul(C.byref(cam), P(uv), len(uv), P(out))
    return out


def inverse_lens(cam, u, v):
    """numpy: distorted pixels (u, v) -> the pinhole pixels of the same camera matrix, by the five-iteration inverse of
    cvUndistortPoints"""
    fx, fy, cx, cy = cam.cameraMatrix[0], cam.cameraMatrix[4], cam.cameraMatrix[2], cam.cameraMatrix[5]
    k1, k2, p1, p2, k3 = list(cam.distCoeffs)
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        ddx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        ddy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - ddx) * icd, (y0 - ddy) * icd
    return x * fx + cx, y * fy + cy


def distort_image(Pimg, cam):
    """what the camera with cam's lens sees where a pinhole camera with the same camera matrix sees Pimg ([H, W] or [H, W, c] uint8):
    the image D whose pixel x_d is Pimg sampled bilinearly (float64, rounded to nearest; the frame's edge repeated outside) at
    K inverse(x_d).  A truly distorted image: straight edges of Pimg are curves in D."""
    Pimg = np.asarray(Pimg)
    Hh, W = Pimg.shape[:2]
    v, u = np.mgrid[0:Hh, 0:W].astype(np.float64)
    xs, ys = inverse_lens(cam, u, v)
    xs, ys = np.clip(xs, 0, W - 1), np.clip(ys, 0, Hh - 1)
    x0, y0 = np.minimum(np.floor(xs).astype(np.int64), W - 2), np.minimum(np.floor(ys).astype(np.int64), Hh - 2)
    ax, ay = xs - x0, ys - y0
    if Pimg.ndim == 3:
        ax, ay = ax[..., None], ay[..., None]
    src = Pimg.astype(np.float64)
    val = (src[y0, x0] * (1 - ax) + src[y0, x0 + 1] * ax) * (1 - ay) + (src[y0 + 1, x0] * (1 - ax) + src[y0 + 1, x0 + 1] * ax) * ay
    return np.rint(val).astype(np.uint8)

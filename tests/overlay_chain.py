"""Overlays for the overlay tests (ocvar_hip_set_overlay / ocvar_hip_render / ocvar_hip_render_records): the host build of
opencv-ar_amd/csrc/overlay_core.h (tests/emul/overlay_emul.cpp) and the sequential host reference the device must match byte
for byte, on frame_kit's guarded frames and marker records.  Shared by tests/test_overlay_cpu.py and tests/test_gpu_overlay.py."""
import ctypes as C

import numpy as np

from frame_kit import FORMATS
from helpers import P
from hostbuild import host_core


def build_emul():
    L = host_core("overlay_emul")
    L.overlay_render_frame_emul.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.overlay_grey_emul.argtypes = [C.c_int] * 3
    return L


def host_render(L, frames, recs, counts, overlays, per_frame=None, buf=None):
    """the host core on a copy of frames.buf (or of buf): recs [n, stride] records, counts [n], overlays {template id (-1: default):
    H x W x 4 uint8} -> (the rendered buffer, records drawn per frame)"""
    out = (frames.buf if buf is None else buf).copy()
    recs = np.ascontiguousarray(recs)
    stride = recs.shape[1] if per_frame is None else per_frame
    assert recs.shape[1] == stride
    tex = [np.ascontiguousarray(v, np.uint8) for v in overlays.values()]
    ptrs = (C.c_void_p * max(len(tex), 1))(*[t.ctypes.data for t in tex])
    tw = np.array([t.shape[1] for t in tex] + [0], np.int32)
    th = np.array([t.shape[0] for t in tex] + [0], np.int32)
    tids = np.array(list(overlays.keys()) + [0], np.int32)
    drawn = []
    for f in range(frames.n):
        drawn.append(L.overlay_render_frame_emul(out.ctypes.data + frames.offset(f), frames.width, frames.height, frames.row_stride,
                                                 frames.fmt, recs[f].ctypes.data, int(counts[f]), stride, ptrs, P(tw), P(th), P(tids),
                                                 len(tex)))
    return out, drawn


def blend(c, a, d):
    """the blend formula on integer arrays"""
    c, a, d = (np.asarray(v, np.int64) for v in (c, a, d))
    return (c * a + d * (255 - a) + 127) // 255


def grey_of(b, g, r):
    """the library's BGR-to-grey integer formula"""
    b, g, r = (np.asarray(v, np.int64) for v in (b, g, r))
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def colour_in_format(rgba, fmt):
    """the colour bytes a frame pixel in format fmt takes from R G B A colours [..., 4]: [..., 3] in memory order, [..., 1] for gray"""
    rgba = np.asarray(rgba, np.int64)
    R, G, B = rgba[..., 0], rgba[..., 1], rgba[..., 2]
    fmt = FORMATS[fmt] if isinstance(fmt, str) else fmt
    if fmt == 4:
        return grey_of(B, G, R)[..., None]
    return np.stack([B, G, R] if fmt in (0, 2) else [R, G, B], axis=-1)


def random_overlay(rng, w, h, alpha="mixed"):
    """an h x w RGBA image; alpha 'mixed': zeros, 255s and everything between, or a constant"""
    o = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha == "mixed":
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        sel = rng.integers(0, 4, (h, w))
        a[sel == 0] = 0
        a[sel == 1] = 255
        o[..., 3] = a
    else:
        o[..., 3] = alpha
    return o


def inside_quad(quad, width, height):
    """signed distance-like margin of every pixel centre of a width x height frame to the convex quad [4, 2]: the smallest of the
    four edge distances, positive inside"""
    q = np.asarray(quad, np.float64).reshape(4, 2)
    area2 = sum(q[i, 0] * q[(i + 1) % 4, 1] - q[(i + 1) % 4, 0] * q[i, 1] for i in range(4))
    ys, xs = np.mgrid[0:height, 0:width]
    d = np.full((height, width), np.inf)
    for i in range(4):
        a, b = q[i], q[(i + 1) % 4]
        e = b - a
        n = np.hypot(*e)
        s = (e[0] * (ys - a[1]) - e[1] * (xs - a[0])) / n
        d = np.minimum(d, s if area2 > 0 else -s)
    return d

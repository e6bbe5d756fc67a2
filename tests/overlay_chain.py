"""Overlays for the overlay tests (ocvar_hip_set_overlay / ocvar_hip_render / ocvar_hip_render_records): the host build of
opencv-ar_amd/csrc/overlay_core.h (tests/emul/overlay_emul.cpp), frames with guard bytes in the row padding and around the
buffer, hand-made marker records, and the sequential host reference the device must match byte for byte.  Shared by
tests/test_overlay_cpu.py and tests/test_gpu_overlay.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import helpers as H
from helpers import P

CSRC = os.path.join(H.PKG, "csrc")
FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "gray": 4}
BPP = {0: 3, 1: 3, 2: 4, 3: 4, 4: 1}
MARKER_DTYPE = np.dtype([("glMatrix", "<f8", (16,)), ("templateId", "<i4"), ("markerId", "<i4"), ("score", "<f8"),
                         ("square", "<f4", (8,)), ("aspectRatio", "<f8")], align=True)
assert MARKER_DTYPE.itemsize == 184
GUARD = 0xA5
LEAD = 64   # guard bytes in front of the first frame and behind the last one (a multiple of 4: the frames stay aligned)


def build_emul(out_dir):
    so = os.path.join(str(out_dir), "liboverlay_emul.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           "-I" + os.path.join(H.ROOT, "include"), "-shared", "-o", so,
                           os.path.join(H.ROOT, "tests", "emul", "overlay_emul.cpp")])
    L = C.CDLL(so)
    L.overlay_render_frame_emul.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.overlay_grey_emul.argtypes = [C.c_int] * 3
    return L


def records(squares, template_ids=None, scores=None):
    """[k] marker records with the given squares (k x 8 or k x 4 x 2), template ids (default 0) and scores (default 1)"""
    sq = np.asarray(squares, np.float32).reshape(-1, 8)
    r = np.zeros(len(sq), MARKER_DTYPE)
    r["square"] = sq
    r["templateId"] = 0 if template_ids is None else template_ids
    r["score"] = 1.0 if scores is None else scores
    r["markerId"] = np.arange(len(sq))
    return r


def axis_square(x0, y0, w, h):
    """the axis-aligned square whose corners are the pixel centres (x0, y0) .. (x0 + w - 1, y0 + h - 1), corner 0 top-left, clockwise
    on screen"""
    return [x0, y0, x0 + w - 1, y0, x0 + w - 1, y0 + h - 1, x0, y0 + h - 1]


class Frames:
    """n frames of height x width pixels in format fmt inside one guarded byte buffer: rows row_stride apart, frames frame_stride
    apart, every byte that is no pixel = GUARD.  `buf` is the whole buffer, `view(f)` frame f's [height, width, bpp] pixels."""

    def __init__(self, n, width, height, fmt, row_pad=0, frame_gap=0, seed=0, fill=None):
        self.n, self.width, self.height = n, width, height
        self.fmt = FORMATS[fmt] if isinstance(fmt, str) else fmt
        self.bpp = BPP[self.fmt]
        self.row_stride = width * self.bpp + row_pad
        self.frame_stride = self.row_stride * height + frame_gap
        self.buf = np.full(2 * LEAD + n * self.frame_stride, GUARD, np.uint8)
        rng = np.random.default_rng(seed)
        for f in range(n):
            v = self.view(f)
            v[...] = rng.integers(0, 256, v.shape, dtype=np.uint8) if fill is None else fill

    def offset(self, f=0):
        return LEAD + f * self.frame_stride

    def view(self, f, buf=None):
        buf = self.buf if buf is None else buf
        rows = np.lib.stride_tricks.as_strided(buf[self.offset(f):], (self.height, self.width, self.bpp), (self.row_stride, self.bpp, 1))
        return rows

    def pixel_mask(self):
        """True at every byte of the buffer that belongs to a pixel"""
        m = np.zeros(self.buf.size, bool)
        for f in range(self.n):
            self.view(f, m)[...] = True
        return m


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

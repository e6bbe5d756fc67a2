"""YUV conversion for the yuv tests (ocvar_hip_yuv_to_frames / ocvar_hip_frames_to_yuv): the host build of
opencv-ar_amd/csrc/yuv_core.h (tests/emul/yuv_emul.cpp), guarded buffers of NV12, I420, YUYV and UYVY frames next to
frame_kit's guarded frames, and a numpy restatement of the equations.  Shared by tests/test_yuv_cpu.py and
tests/test_gpu_yuv.py."""
import ctypes as C

import numpy as np

import overlay_chain as OC
from frame_kit import FORMATS, GUARD, LEAD
from hostbuild import host_core

LAYOUTS = {"nv12": 0, "i420": 1, "yuyv": 2, "uyvy": 3}
MATRICES = {"bt601": 0, "bt709": 1}
# one lane, a full lane, a lane with a 2-pixel tail, both sides of a wave's 512-pixel span, a second workgroup
SIZES = [(2, 2), (4, 2), (6, 4), (8, 2), (10, 6), (510, 2), (512, 4), (514, 2), (1026, 2)]
COEF_NAMES = ["cy", "cub", "cug", "cvg", "cvr", "ry", "gy", "by", "ru", "gu", "bu", "rv", "gv", "bv"]
# the tables as the issue states them
COEF = {
    "bt601": dict(cy=1220542, cub=2116026, cug=-409993, cvg=-852492, cvr=1673527, ry=269484, gy=528482, by=102760,
                  ru=-155188, gu=-305135, bu=460324, rv=460324, gv=-385875, bv=-74448),
    "bt709": dict(cy=1220945, cvr=1879825, cub=2215014, cug=-223607, cvg=-558796, ry=191455, gy=644067, by=65019,
                  ru=-105533, gu=-355018, bu=460551, rv=460551, gv=-418321, bv=-42230),
}


def build_emul():
    L = host_core("yuv_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.yuv_to_frames_emul.argtypes = [i, i, vp, vp, vp, ll, ll, ll, vp, ll, ll, i, i, i, i]
    L.frames_to_yuv_emul.argtypes = [i, i, vp, vp, vp, ll, ll, ll, vp, ll, ll, i, i, i, i]
    L.yuv_to_bgr_all_emul.argtypes = [i, vp]
    L.bgr_to_yuv_all_emul.argtypes = [i, i, vp]
    L.yuv_chroma_emul.argtypes = [i, i, vp, i, vp]
    L.yuv_coef_emul.argtypes = [i, vp]
    return L


class Yuv:
    """n frames of width x height in a YUV layout inside one guarded byte buffer: per frame the Y (or packed) plane, then the chroma
    plane(s), every row followed by padding, every frame by a gap; every byte that is no sample = GUARD.  aligned: every plane
    offset, pitch and the frame stride are multiples of 4 (and the lead); else the lead is odd and the paddings are 3 and 1."""

    def __init__(self, n, width, height, layout, aligned=False, seed=None):
        self.n, self.width, self.height = n, width, height
        self.layout = LAYOUTS[layout] if isinstance(layout, str) else layout
        self.s420 = self.layout in (0, 1)
        assert width % 2 == 0 and (height % 2 == 0 or not self.s420)
        self.aligned = aligned

        def pitch(row_bytes, odd_pad):
            return row_bytes + 4 + (-row_bytes) % 4 if aligned else row_bytes + odd_pad

        self.lead = LEAD if aligned else LEAD + 1
        y_bytes = width if self.s420 else 2 * width
        self.y_pitch = pitch(y_bytes, 3)
        self.planes = [(0, y_bytes, height, self.y_pitch)]   # (offset in the frame, bytes per row, rows, pitch)
        self.c_pitch, end = 0, self.y_pitch * height
        if self.s420:
            c_bytes = width if self.layout == 0 else width // 2
            self.c_pitch = pitch(c_bytes, 1)
            for _ in range(1 if self.layout == 0 else 2):
                end += 0 if aligned else 2   # (a gap between the planes: a chroma offset)
                self.planes.append((end, c_bytes, height // 2, self.c_pitch))
                end += self.c_pitch * (height // 2)
        self.frame_stride = end + (8 if aligned else 5)
        self.buf = np.full(self.lead + n * self.frame_stride + LEAD, GUARD, np.uint8)
        if aligned:
            assert all(v % 4 == 0 for v in [self.lead, self.frame_stride, self.y_pitch, self.c_pitch] + [p[0] for p in self.planes])
        if seed is not None:
            rng = np.random.default_rng(seed)
            m = self.sample_mask()
            self.buf[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)

    def offset(self, f=0, plane=0):
        return self.lead + f * self.frame_stride + self.planes[plane][0]

    def plane_view(self, f, plane, buf=None):
        buf = self.buf if buf is None else buf
        _, row_bytes, rows, pitch = self.planes[plane]
        return np.lib.stride_tricks.as_strided(buf[self.offset(f, plane):], (rows, row_bytes), (pitch, 1))

    def sample_mask(self):
        m = np.zeros(self.buf.size, bool)
        for f in range(self.n):
            for k in range(len(self.planes)):
                self.plane_view(f, k, m)[...] = True
        return m

    def pointers(self, base):
        """(y, c0, c1) of frame 0 with the buffer at address base; None for a plane the layout has not"""
        p = [base + self.offset(0, k) for k in range(len(self.planes))]
        return tuple(p + [None] * (3 - len(p)))

    def samples(self, f, buf=None):
        """frame f's samples in one form for every layout: Y [H, W], U and V [H / 2 or H, W / 2]"""
        v = [self.plane_view(f, k, buf) for k in range(len(self.planes))]
        if self.layout == 0:
            return v[0].copy(), v[1][:, 0::2].copy(), v[1][:, 1::2].copy()
        if self.layout == 1:
            return v[0].copy(), v[1].copy(), v[2].copy()
        yo, uo, vo = (0, 1, 3) if self.layout == 2 else (1, 0, 2)
        return v[0][:, yo::2].copy(), v[0][:, uo::4].copy(), v[0][:, vo::4].copy()

    def put_samples(self, f, Y, U, V):
        v = [self.plane_view(f, k) for k in range(len(self.planes))]
        if self.layout == 0:
            v[0][...], v[1][:, 0::2], v[1][:, 1::2] = Y, U, V
        elif self.layout == 1:
            v[0][...], v[1][...], v[2][...] = Y, U, V
        else:
            yo, uo, vo = (0, 1, 3) if self.layout == 2 else (1, 0, 2)
            v[0][:, yo::2], v[0][:, uo::4], v[0][:, vo::4] = Y, U, V


def code(table, v):
    return table[v] if isinstance(v, str) else v


def host_to_frames(L, yuv, matrix, dst, buf=None):
    """the host core: the YUV frames of yuv.buf (or buf) -> dst's buffer, filled"""
    assert (yuv.n, yuv.width, yuv.height) == (dst.n, dst.width, dst.height)
    src = np.ascontiguousarray(yuv.buf if buf is None else buf)
    out = dst.buf.copy()
    y, c0, c1 = yuv.pointers(src.ctypes.data)
    L.yuv_to_frames_emul(yuv.layout, code(MATRICES, matrix), y, c0, c1, yuv.y_pitch, yuv.c_pitch, yuv.frame_stride,
                         out.ctypes.data + dst.offset(0), dst.row_stride, dst.frame_stride, yuv.width, yuv.height, dst.fmt, yuv.n)
    return out


def host_to_yuv(L, src, matrix, yuv, buf=None):
    """the host core: the frames of src.buf (or buf) -> yuv's buffer, filled"""
    assert (yuv.n, yuv.width, yuv.height) == (src.n, src.width, src.height)
    sb = np.ascontiguousarray(src.buf if buf is None else buf)
    out = yuv.buf.copy()
    y, c0, c1 = yuv.pointers(out.ctypes.data)
    L.frames_to_yuv_emul(yuv.layout, code(MATRICES, matrix), y, c0, c1, yuv.y_pitch, yuv.c_pitch, yuv.frame_stride,
                         sb.ctypes.data + src.offset(0), src.row_stride, src.frame_stride, yuv.width, yuv.height, src.fmt, yuv.n)
    return out


# ---- numpy restatement of the equations (int64 throughout; >> on numpy ints is the floor shift) ---------------------------------------

def clamp(v):
    return np.clip(v, 0, 255)


def np_yuv_to_bgr(matrix, Y, U, V):
    k = COEF[matrix]
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    u, v = U - 128, V - 128
    y = np.maximum(Y - 16, 0) * k["cy"]
    R = clamp((y + (1 << 19) + k["cvr"] * v) >> 20)
    G = clamp((y + (1 << 19) + k["cvg"] * v + k["cug"] * u) >> 20)
    B = clamp((y + (1 << 19) + k["cub"] * u) >> 20)
    return B, G, R


def np_luma(matrix, B, G, R):
    k = COEF[matrix]
    B, G, R = (np.asarray(a, np.int64) for a in (B, G, R))
    return clamp((k["ry"] * R + k["gy"] * G + k["by"] * B + (1 << 19) + (16 << 20)) >> 20)


def np_chroma(matrix, sB, sG, sR, log2n):
    k = COEF[matrix]
    sB, sG, sR = (np.asarray(a, np.int64) for a in (sB, sG, sR))
    bias = ((1 << 19) << log2n) + (128 << (20 + log2n))
    U = clamp((k["ru"] * sR + k["gu"] * sG + k["bu"] * sB + bias) >> (20 + log2n))
    V = clamp((k["rv"] * sR + k["gv"] * sG + k["bv"] * sB + bias) >> (20 + log2n))
    return U, V


def np_pixels(fmt, B, G, R):
    """[H, W, bpp] uint8 pixels of a colour in format fmt as a conversion target writes them"""
    fmt = code(FORMATS, fmt)
    if fmt == 4:
        return OC.grey_of(B, G, R)[..., None].astype(np.uint8)
    ch = [B, G, R] if fmt in (0, 2) else [R, G, B]
    if fmt in (2, 3):
        ch = ch + [np.full_like(B, 255)]
    return np.stack(ch, -1).astype(np.uint8)


def np_colour(fmt, px):
    """B, G, R (int64) of [H, W, bpp] pixels in format fmt as a conversion source reads them"""
    fmt = code(FORMATS, fmt)
    px = np.asarray(px, np.int64)
    if fmt == 4:
        return px[..., 0], px[..., 0], px[..., 0]
    return (px[..., 0], px[..., 1], px[..., 2]) if fmt in (0, 2) else (px[..., 2], px[..., 1], px[..., 0])


def np_frame_to_pixels(matrix, fmt, Y, U, V):
    """one frame's samples (Yuv.samples) -> its [H, W, bpp] pixels: every chroma sample repeated over its block"""
    ry = Y.shape[0] // U.shape[0]
    Uf, Vf = (np.repeat(np.repeat(c, ry, 0), 2, 1) for c in (U, V))
    return np_pixels(fmt, *np_yuv_to_bgr(matrix, Y, Uf, Vf))


def np_pixels_to_frame(matrix, fmt, px, s420):
    """[H, W, bpp] pixels -> the frame's samples Y, U, V"""
    B, G, R = np_colour(fmt, px)
    Hh, W = B.shape
    bh = 2 if s420 else 1
    sums = [c.reshape(Hh // bh, bh, W // 2, 2).sum((1, 3)) for c in (B, G, R)]
    U, V = np_chroma(matrix, *sums, log2n=bh)   # (2^bh pixels per block: 4 or 2)
    return np_luma(matrix, B, G, R).astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)

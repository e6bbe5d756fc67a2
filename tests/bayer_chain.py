"""Bayer demosaic for the bayer tests (ocvar_hip_bayer_to_frames): the host build of opencv-ar_amd/csrc/bayer_core.h
(tests/emul/bayer_emul.cpp), guarded buffers of raw mosaics next to frame_kit's guarded frames, mosaic() to make a raw frame of a
colour one, and a numpy restatement of the whole rule on reflect-padded planes and shifted sums that shares no code with the core.
Shared by tests/test_bayer_cpu.py and tests/test_gpu_bayer.py."""
import ctypes as C

import numpy as np

import yuv_chain as YC
from frame_kit import BPP, FORMATS, GUARD, LEAD
from hostbuild import host_core

PATTERNS = {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}
# the top-left 2 x 2 of each pattern, row by row, as channel codes: 0 B, 1 G, 2 R
TILES = {"rggb": [[2, 1], [1, 0]], "grbg": [[1, 2], [0, 1]], "gbrg": [[1, 0], [2, 1]], "bggr": [[0, 1], [1, 2]]}
DEPTHS = [8, 10, 12, 16]
# the sizes of the issue's CPU sweep: the smallest frames, odd sides, a lane's span of 8 and its neighbours, a wave's span of 512 + 1
SIZES = [(2, 2), (2, 3), (3, 2), (3, 3), (5, 4), (9, 7), (17, 6), (513, 5)]
MAX_GAIN = 16383
PAIRS, MAX_PAIRS = 4, 64   # row pairs a lane of the kernels marches down: the default, the most (bayer_core.h; OCVAR_TUNE_BAYER_PAIRS)


class Params(C.Structure):  # OcvarBayerParams
    _fields_ = [("pattern", C.c_int), ("bits", C.c_int), ("black", C.c_int), ("gain_b", C.c_int), ("gain_g", C.c_int), ("gain_r", C.c_int)]


def params(pattern="rggb", bits=8, black=0, gains=(1024, 1024, 1024)):
    """gains: (blue, green, red) in 1/1024"""
    return Params(PATTERNS[pattern] if isinstance(pattern, str) else pattern, bits, black, gains[0], gains[1], gains[2])


def as_tuple(p):
    return (p.pattern, p.bits, p.black, p.gain_b, p.gain_g, p.gain_r)


def build_emul():
    L = host_core("bayer_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.bayer_to_frames_emul.argtypes = [vp, ll, ll, vp, ll, ll, i, i, i, i, vp]
    L.bayer_lanes_emul.argtypes = [vp, ll, ll, vp, ll, ll, i, i, i, i, vp, i]
    L.bayer_pairs_emul.argtypes = [i]
    L.bayer_cut_emul.argtypes = [vp, ll, i, i, vp]
    L.bayer_default_params_emul.argtypes = [vp]
    L.bayer_params_bad_emul.argtypes = [vp]
    L.bayer_pattern_at_emul.argtypes = [i, i, i]
    L.bayer_colour_at_emul.argtypes = [i, i, i]
    L.bayer_reflect_emul.argtypes = [i, i]
    L.bayer_balance_emul.argtypes = [i, i, i, i]
    L.bayer_reduce_emul.argtypes = [i, i]
    return L


def sample_bytes(bits):
    return 2 if bits > 8 else 1


class Raw:
    """n raw mosaics of width x height samples of `bits` bits (bytes, or little-endian 16-bit words) inside one guarded byte buffer:
    every row followed by padding, every frame by a gap; every byte that is no sample = GUARD.  aligned: the lead, the pitch and the
    frame stride are multiples of 4; else, with bytes, an odd lead and an odd pitch, and with words an even lead, pitch and frame
    stride that keep the first sample off a multiple of 4.  seed: random bytes in every sample (a word's bits above `bits` too, which
    the definition masks away)."""

    def __init__(self, n, width, height, bits, aligned=False, seed=None):
        self.n, self.width, self.height, self.bits, self.aligned = n, width, height, bits, aligned
        self.sb = sample_bytes(bits)
        self.row_bytes = self.sb * width
        if aligned:
            self.lead, self.row_stride, gap = LEAD, self.row_bytes + 4 + (-self.row_bytes) % 4, 8
        elif self.sb == 1:
            self.lead, self.row_stride, gap = LEAD + 1, self.row_bytes + 1 + self.row_bytes % 2, 5   # (an odd pitch)
        else:
            self.lead, self.row_stride, gap = LEAD + 2, self.row_bytes + 2, 6
        self.frame_stride = self.row_stride * height + gap
        self.buf = np.full(self.lead + n * self.frame_stride + LEAD, GUARD, np.uint8)
        if aligned:
            assert all(v % 4 == 0 for v in (self.lead, self.row_stride, self.frame_stride))
        else:
            assert self.lead % 4 != 0 and all(v % self.sb == 0 for v in (self.lead, self.row_stride, self.frame_stride))
            assert self.sb == 2 or self.row_stride % 2 == 1
        if seed is not None:
            rng = np.random.default_rng(seed)
            m = self.sample_mask()
            self.buf[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)

    def offset(self, f=0):
        return self.lead + f * self.frame_stride

    def view(self, f, buf=None):
        """frame f's bytes [height, row_bytes]"""
        buf = self.buf if buf is None else buf
        return np.lib.stride_tricks.as_strided(buf[self.offset(f):], (self.height, self.row_bytes), (self.row_stride, 1))

    def sample_mask(self):
        m = np.zeros(self.buf.size, bool)
        for f in range(self.n):
            self.view(f, m)[...] = True
        return m

    def put(self, f, samples):
        """[height, width] integers -> frame f's bytes or words"""
        s = np.asarray(samples)
        self.view(f)[...] = s.astype(np.uint8) if self.sb == 1 else np.ascontiguousarray(s.astype("<u2")).view(np.uint8).reshape(self.height, -1)

    def words(self, f, buf=None):
        """frame f's bytes or whole 16-bit words as int64 [height, width], before the mask"""
        v = np.ascontiguousarray(self.view(f, buf))
        return (v if self.sb == 1 else v.view("<u2")).astype(np.int64)


def host_demosaic(L, raw, dst, p=None, buf=None, lanes=0):
    """the host core (lanes > 0: through the kernels' lane arithmetic, marching down strips of `lanes` row pairs): the mosaics of
    raw.buf (or buf) -> dst's buffer, filled"""
    assert (raw.n, raw.width, raw.height) == (dst.n, dst.width, dst.height)
    src = np.ascontiguousarray(raw.buf if buf is None else buf)
    out = dst.buf.copy()
    args = (src.ctypes.data + raw.offset(0), raw.row_stride, raw.frame_stride, out.ctypes.data + dst.offset(0), dst.row_stride, dst.frame_stride,
            raw.width, raw.height, dst.fmt, raw.n, None if p is None else C.addressof(p))
    rc = L.bayer_lanes_emul(*args, lanes) if lanes else L.bayer_to_frames_emul(*args)
    assert rc == 0, rc
    return out


def host_demosaic_image(L, samples, p, fmt="bgr"):
    """the host core on one contiguous [H, W] mosaic (uint8, or uint16 when p.bits > 8) -> [H, W, bpp] pixels"""
    s = np.ascontiguousarray(samples, np.uint8 if p.bits == 8 else "<u2")
    h, w = s.shape
    bpp = BPP[FORMATS[fmt]]
    out = np.zeros((h, w, bpp), np.uint8)
    rc = L.bayer_to_frames_emul(s.ctypes.data, w * s.itemsize, 0, out.ctypes.data, w * bpp, 0, w, h, FORMATS[fmt], 1, C.addressof(p))
    assert rc == 0, rc
    return out


# ---- numpy: the mosaic of a colour frame, and the restatement of the rule ------------------------------------------------------------------

def colour_map(pattern, h, w):
    """[h, w] channel codes (0 B, 1 G, 2 R) of a mosaic in `pattern` (a name), its 2 x 2 tile repeated"""
    return np.tile(np.array(TILES[pattern]), ((h + 1) // 2, (w + 1) // 2))[:h, :w]


def mosaic(bgr, pattern, bits=8):
    """[H, W, 3] uint8 B G R -> the [H, W] raw frame a sensor in `pattern` would deliver: at every site the channel of its colour,
    moved up to `bits` bits (v << (bits - 8): the reduction gives v back); uint8, or uint16 for bits > 8"""
    bgr = np.asarray(bgr)
    h, w = bgr.shape[:2]
    s = np.take_along_axis(bgr.astype(np.int64), colour_map(pattern, h, w)[..., None], 2)[..., 0] << (bits - 8)
    return s.astype(np.uint8 if bits == 8 else np.uint16)


def np_balance(raw, cm, bits, black, gains):
    s = np.asarray(raw, np.int64) & ((1 << bits) - 1)
    return np.minimum((1 << bits) - 1, (np.maximum(s - black, 0) * np.asarray(gains, np.int64)[cm] + 512) >> 10)


def np_demosaic(raw, pattern, bits=8, black=0, gains=(1024, 1024, 1024), fmt="bgr"):
    """[H, W] raw words (before the mask) -> [H, W, bpp] uint8 by the definition, restated on whole planes: balance, a reflect pad of
    one sample (numpy's 'reflect' does not repeat the edge), the four sums as shifted slices, a choice per site kind, the reduction"""
    h, w = np.asarray(raw).shape
    wide = colour_map(pattern, h + 1, w + 1)
    cm, right = wide[:h, :w], wide[:h, 1:]       # a site's colour, and its right neighbour's: the colour of the row's other sites
    P = np.pad(np_balance(raw, cm, bits, black, gains), 1, mode="reflect")
    c, N, S, Wt, E = P[1:-1, 1:-1], P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]
    cross = (N + S + Wt + E + 2) >> 2
    diag = (P[:-2, :-2] + P[:-2, 2:] + P[2:, :-2] + P[2:, 2:] + 2) >> 2
    hor, ver = (Wt + E + 1) >> 1, (N + S + 1) >> 1
    G = np.where(cm == 1, c, cross)
    R = np.where(cm == 2, c, np.where(cm == 0, diag, np.where(right == 2, hor, ver)))
    B = np.where(cm == 0, c, np.where(cm == 2, diag, np.where(right == 0, hor, ver)))
    if bits > 8:
        B, G, R = (np.minimum(255, (v + (1 << (bits - 9))) >> (bits - 8)) for v in (B, G, R))
    return YC.np_pixels(fmt, B, G, R)


def np_demosaic_params(raw, p, fmt="bgr"):
    name = {v: k for k, v in PATTERNS.items()}[p.pattern]
    return np_demosaic(raw, name, p.bits, p.black, (p.gain_b, p.gain_g, p.gain_r), fmt)


# non-default black levels and gains (blue, green, red in 1/1024) per depth: a gain of 0, the largest gain, black = the largest sample
def knobs(bits):
    top = (1 << bits) - 1
    return [(0, (1024, 1024, 1024)), (top // 16, (1500, 1024, 1900)), (3, (0, 700, MAX_GAIN)), (top, (1024, 2048, 512)), (0, (MAX_GAIN, MAX_GAIN, 0))]


# ---- the chain through the oracle --------------------------------------------------------------------------------------------------------

def corner_set_distance(a, b):
    """the distance of two squares (8 floats each) as sets of four corners, whatever their order: the largest max-abs distance
    from a corner of either to the nearest corner of the other"""
    a, b = np.asarray(a, np.float64).reshape(4, 1, 2), np.asarray(b, np.float64).reshape(1, 4, 2)
    d = np.abs(a - b).max(2)
    return max(d.min(0).max(), d.min(1).max())


def corners_moved(found, truth):
    """for every record of truth the smallest corner_set_distance to a record of found; inf without one"""
    return [min([corner_set_distance(m.square, t.square) for m in found] or [np.inf]) for t in truth]

"""Grey levels for the levels tests (ocvar_hip_levels): the host build of opencv-ar_amd/csrc/levels_core.h (tests/emul/levels_emul.cpp),
a numpy restatement of the definition that shares no code with it, guarded frames (frame_kit.pix_layout), the
cases the CPU and GPU tests share, and the exposure chain through the oracle on the library's own synthetic scenes.  Shared by
tests/test_levels_cpu.py and tests/test_gpu_levels.py."""
import ctypes as C

import numpy as np

import helpers as H
import overlay_chain as OC
from frame_kit import FORMATS, GUARD, pix_layout
from hostbuild import host_core

FMT_NAMES = {v: k for k, v in FORMATS.items()}
# levels.hip: a workgroup of the histogram kernel counts SLAB_ROWS rows of a tile, one of the apply kernel a rectangle of at most
# SEG_W x SEG_H pixels inside one cell of the tile-centre lattice; the workspace takes WS_FRAMES frames a round (levels_core.h;
# tests/test_levels_cpu.py compares these with the core's)
SLAB_ROWS, SEG_W, SEG_H, WS_FRAMES, MAX_TILES = 32, 256, 32, 256, 64
WS_BYTES = WS_FRAMES * MAX_TILES * (1024 + 256)


class Params(C.Structure):  # OcvarLevelsParams
    _fields_ = [("tiles_x", C.c_int), ("tiles_y", C.c_int), ("low_ppm", C.c_int), ("high_ppm", C.c_int), ("max_gain_q8", C.c_int)]


def params(tiles=(1, 1), low_ppm=10000, high_ppm=10000, max_gain_q8=2048):
    return Params(tiles[0], tiles[1], low_ppm, high_ppm, max_gain_q8)


def as_tuple(p):
    return (p.tiles_x, p.tiles_y, p.low_ppm, p.high_ppm, p.max_gain_q8)


def build_emul():
    L = host_core("levels_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.levels_emul.argtypes = [vp, i, i, ll, ll, i, vp, ll, ll, i, vp, vp, vp]
    L.levels_default_params_emul.argtypes = [vp]
    L.levels_params_bad_emul.argtypes = [vp, i, i]
    L.levels_lut_emul.argtypes = [vp, vp, vp]
    L.levels_bounds_emul.argtypes = [vp, vp, vp]
    L.levels_axis_emul.argtypes = [i, i, i, vp]
    L.levels_grey_emul.argtypes = [i, i, i, i]
    L.levels_segments_emul.argtypes = [i, i, i, vp]
    L.levels_ws_bytes_emul.restype = ll
    return L


def dst_layout(src, aligned, fill=GUARD, n=None):
    """guarded GRAY planes of the frames' size"""
    return pix_layout(src.n if n is None else n, src.width, src.height, "gray", aligned, fill=fill)


def host_levels(L, src, dst, p=None, buf=None, want_luts=False):
    """the host core: the frames of src.buf (or buf) -> (return code, dst's buffer afterwards[, LUTs [n, tiles, 256]])"""
    sb = np.ascontiguousarray(src.buf if buf is None else buf)
    out = dst.buf.copy()
    tiles = 1 if p is None else max(p.tiles_x * p.tiles_y, 1)
    luts = np.zeros((src.n, tiles, 256), np.uint8)
    rc = L.levels_emul(sb.ctypes.data + src.offset(0), src.width, src.height, src.row_stride, src.frame_stride, src.fmt, out.ctypes.data + dst.offset(0),
                       dst.row_stride, dst.frame_stride, src.n, None if p is None else C.addressof(p), luts.ctypes.data if want_luts else None, None)
    return (rc, out, luts) if want_luts else (rc, out)


def host_levels_image(L, img, p=None, fmt=None):
    """the host core on one contiguous [H, W] grey or [H, W, C] image -> the [H, W] plane"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    code = FORMATS[fmt] if fmt else {1: FORMATS["gray"], 3: FORMATS["bgr"], 4: FORMATS["bgra"]}[ch]
    out = np.zeros((h, w), np.uint8)
    rc = L.levels_emul(img.ctypes.data, w, h, w * ch, w * h * ch, code, out.ctypes.data, w, w * h, 1, None if p is None else C.addressof(p), None, None)
    assert rc == 0, rc
    return out


# ---- numpy restatement of the definition --------------------------------------------------------------------------------------------------

def np_grey(px, fmt):
    """[..., bpp] pixels in format fmt (a name) -> [...] the library's grey"""
    px = np.asarray(px)
    if fmt == "gray":
        return px[..., 0].astype(np.uint8)
    b, r = (px[..., 0], px[..., 2]) if fmt in ("bgr", "bgra") else (px[..., 2], px[..., 0])
    return OC.grey_of(b, px[..., 1], r).astype(np.uint8)


def np_edges(extent, tiles):
    return np.array([(i * extent) // tiles for i in range(tiles + 1)], np.int64)


def np_bounds(g, low_ppm, high_ppm):
    """(lo, hi) of the grey values g before the gain cap"""
    hist = np.bincount(np.asarray(g).ravel(), minlength=256).astype(np.int64)
    n = int(hist.sum())
    k_lo, k_hi = (n * low_ppm) // 1000000, (n * high_ppm) // 1000000
    at_most = np.cumsum(hist)                   # #{g <= v}
    at_least = np.cumsum(hist[::-1])[::-1]      # #{g >= v}
    return int(np.flatnonzero(at_most > k_lo)[0]), int(np.flatnonzero(at_least > k_hi)[-1])


def np_cap(lo, hi, max_gain_q8):
    minr = (255 * 256 + max_gain_q8 - 1) // max_gain_q8
    if hi - lo < minr:
        lo = min(max((lo + hi - minr) >> 1, 0), 255 - minr)
        hi = lo + minr
    return lo, hi


def np_lut(g, low_ppm, high_ppm, max_gain_q8):
    lo, hi = np_cap(*np_bounds(g, low_ppm, high_ppm), max_gain_q8)
    v = np.arange(256, dtype=np.int64)
    return np.minimum(np.maximum((v - lo) * 510 + (hi - lo), 0) // (2 * (hi - lo)), 255)


def np_axis(extent, tiles):
    """for every pixel of an axis: (i0, i1, weight of i1)"""
    e = np_edges(extent, tiles)
    c2 = e[:-1] + e[1:]
    p = 2 * np.arange(extent, dtype=np.int64) + 1
    i0 = np.clip(np.searchsorted(c2, p, side="right") - 1, 0, max(tiles - 2, 0))
    i1 = np.minimum(i0 + 1, tiles - 1)
    den = np.where(i1 > i0, c2[i1] - c2[i0], 1)
    w = np.where(i1 > i0, np.clip(((p - c2[i0]) * 256) // den, 0, 256), 0)
    return i0, i1, w


def np_levels(grey, tiles=(1, 1), low_ppm=10000, high_ppm=10000, max_gain_q8=2048):
    """[H, W] uint8 grey -> [H, W] uint8 by the definition, restated with numpy arrays"""
    grey = np.asarray(grey, np.uint8)
    h, w = grey.shape
    tx, ty = tiles
    xe, ye = np_edges(w, tx), np_edges(h, ty)
    luts = np.zeros((ty, tx, 256), np.int64)
    for j in range(ty):
        for i in range(tx):
            luts[j, i] = np_lut(grey[ye[j]:ye[j + 1], xe[i]:xe[i + 1]], low_ppm, high_ppm, max_gain_q8)
    i0, i1, wx = np_axis(w, tx)
    j0, j1, wy = np_axis(h, ty)
    g = grey.astype(np.int64)
    J0, J1, WY = j0[:, None], j1[:, None], wy[:, None]
    I0, I1, WX = i0[None, :], i1[None, :], wx[None, :]
    top = luts[J0, I0, g] * (256 - WX) + luts[J0, I1, g] * WX
    bot = luts[J1, I0, g] * (256 - WX) + luts[J1, I1, g] * WX
    return ((top * (256 - WY) + bot * WY + 32768) >> 16).astype(np.uint8)


def np_levels_params(grey, p):
    return np_levels(grey, (p.tiles_x, p.tiles_y), p.low_ppm, p.high_ppm, p.max_gain_q8)


# ---- the cases the CPU and GPU tests share -----------------------------------------------------------------------------------------------

# (width, height, tiles): 37 x 23 under three grids, the smallest frames, one-pixel tiles, an 8 x 8 grid on 16 x 16
SHAPES = [(37, 23, (1, 1)), (37, 23, (4, 3)), (37, 23, (5, 2)), (1, 1, (1, 1)), (2, 1, (1, 1)), (5, 3, (1, 1)), (7, 3, (7, 1)), (16, 16, (8, 8))]
# (low_ppm, high_ppm, max_gain_q8) next to the defaults
KNOBS = [(10000, 10000, 2048), (0, 0, 2048), (500000, 500000, 2048), (10000, 10000, 256), (10000, 10000, 65280)]


def special_frames(w, h):
    """name -> [h, w] grey: constant frames of 0, 128 and 255 (both clamps of the gain cap), two values, a ramp over 0 .. 255, and a
    frame whose lo exceeds its hi before the cap at 500000 ppm (half 10, half 240)"""
    x = np.arange(w * h).reshape(h, w)
    return {"zeros": np.zeros((h, w), np.uint8), "mid": np.full((h, w), 128, np.uint8), "ones": np.full((h, w), 255, np.uint8),
            "two": np.where((x % 3) == 0, 40, 90).astype(np.uint8), "ramp": ((x * 255) // max(w * h - 1, 1)).astype(np.uint8),
            "halves": np.where(x % 2 == 0, 10, 240).astype(np.uint8)}


# ---- the exposure chain -------------------------------------------------------------------------------------------------------------------

EXPOSURES = ["dark", "bright", "flat", "halfdark", "ramp", "split"]
CHAIN_RECORDS = 14            # oracle records on the undimmed frames
RECOVERY_PX = 2.0
# records recovered out of CHAIN_RECORDS, measured with the numpy restatement: exposure -> (raw, global, 4x4, 8x8)
CHAIN_MEASURED = {"dark": (0, 11, 11, 10), "bright": (0, 13, 12, 10), "flat": (0, 11, 11, 10), "halfdark": (8, 7, 12, 10),
                  "ramp": (5, 9, 12, 10), "split": (0, 0, 10, 9)}
# the bars: one or two below the measured totals
RAW_ZERO = ("dark", "bright", "flat", "split")
GLOBAL_BAR = {"dark": 10, "bright": 10, "flat": 10}
TILED_BAR = {"halfdark": 10, "ramp": 10, "split": 8}
GLOBAL_SPLIT_AT_MOST = 2


def expose(bgr, name):
    """the exposure `name` of a BGR frame: float64 on the bytes, cut back with astype(uint8)"""
    f = bgr.astype(np.float64)
    w = bgr.shape[1]
    left = (np.arange(w) < w // 2)[None, :, None]
    if name == "dark":
        out = f * 0.35
    elif name == "bright":
        out = f * 0.4 + 150
    elif name == "flat":
        out = f * 0.2 + 60
    elif name == "halfdark":
        out = np.where(left, f * 0.3, f)
    elif name == "ramp":
        out = f * np.linspace(0.2, 1.0, w)[None, :, None]
    elif name == "split":
        out = np.where(left, f * 0.3, f * 0.3 + 170)
    else:
        raise ValueError(name)
    return out.astype(np.uint8)


def chain_scenes():
    """[(name, bgr)]: 640 x 480 config 1 frames 0 .. 3, config 0 cut to 320 x 240 with a 2 x 2 grid of markers 40 .. 70 px wide frames
    0 .. 1, 1920 x 1080 config 0 frames 0 .. 1"""
    out = []
    cfg = H.synth_config(1)
    out += [("640x480-%d" % f, H.synth_frame(cfg, f)[0]) for f in range(4)]
    cfg = H.synth_config(0, width=320, height=240, grid_x=2, grid_y=2, side_min=40, side_max=70)
    out += [("320x240-%d" % f, H.synth_frame(cfg, f)[0]) for f in range(2)]
    cfg = H.synth_config(0)
    out += [("1920x1080-%d" % f, H.synth_frame(cfg, f)[0]) for f in range(2)]
    return out


def oracle_on_grey(grey, tpls):
    """the oracle's records on a grey plane (as a BGR frame of three equal channels, whose grey is the plane)"""
    h, w = grey.shape
    return H.oracle_registration(np.repeat(grey[:, :, None], 3, axis=2), tpls, H.oracle_camera(w, h))[0]


def corner_distance(a, b):
    """max-abs distance of two squares (8 floats each) under the best cyclic shift of the corners"""
    a, b = np.asarray(a, np.float64).reshape(4, 2), np.asarray(b, np.float64).reshape(4, 2)
    return min(np.abs(np.roll(a, s, axis=0) - b).max() for s in range(4))


def recovered(found, truth):
    """how many records of truth have a record in found with the same templateId whose corners lie within RECOVERY_PX"""
    return sum(any(m.templateId == t.templateId and corner_distance(m.square, t.square) <= RECOVERY_PX for m in found) for t in truth)

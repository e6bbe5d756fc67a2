"""Resizing for the resize tests (ocvar_hip_resize / ocvar_hip_scale_records): the host build of
opencv-ar_amd/csrc/resize_core.h (tests/emul/resize_emul.cpp), a numpy restatement of the rules that shares no code with it,
guarded frames (frame_kit.pix_layout), and the single-marker scenes of the 4K-in, 1080p-detect chain at
a quarter of that size.  Shared by tests/test_resize_cpu.py and tests/test_gpu_resize.py."""
import ctypes as C

import numpy as np

import helpers as H
import persp_synth as PS
from frame_kit import FORMATS
from hostbuild import host_core

INTERPS = {"nearest": 0, "linear": 1, "area": 2}
MAX_RATIO = 16
KIND_NEAREST, KIND_LINEAR, KIND_BOX, KIND_TABLE = 0, 1, 2, 3
# resize.hip: RESIZE_LANE_PX = 8 destination pixels per lane, 64 lanes per workgroup
LANE_PX, WAVE_PX = 8, 512
# destination widths: 1, 2, a lane's run, run + 1, both sides of a wave's span (513 starts a second workgroup), a third workgroup
DST_WIDTHS = [1, 2, LANE_PX, LANE_PX + 1, WAVE_PX - 1, WAVE_PX, WAVE_PX + 1, 2 * WAVE_PX + 1]
DST_HEIGHTS = [1, 2, 5]


def build_emul():
    L = host_core("resize_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.resize_emul.argtypes = [vp, i, i, ll, ll, vp, i, i, ll, ll, i, i, i]
    L.resize_plan_emul.argtypes = [i, i, i, i, i, vp]
    L.resize_area_span_emul.argtypes = [i, i, i, i, vp, vp]
    L.resize_linear_tap_emul.argtypes = [i, i, i, vp]
    L.resize_coords_emul.argtypes = [vp, i, i, i, vp]
    L.scale_records_emul.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, vp]
    return L


def code(table, v):
    return table[v] if isinstance(v, str) else v


def area_ok(sw, sh, dw, dh):
    return dw <= sw and dh <= sh and sw <= MAX_RATIO * dw and sh <= MAX_RATIO * dh


def host_resize(L, src, dst, interp, buf=None, src_offset=None, src_size=None):
    """the host core: the frames of src.buf (or buf) -> (return code, dst's buffer afterwards); src_offset / src_size: a source
    rectangle (byte offset of its first pixel, its (width, height)) with src's strides"""
    sb = np.ascontiguousarray(src.buf if buf is None else buf)
    out = dst.buf.copy()
    sw, sh = (src.width, src.height) if src_size is None else src_size
    rc = L.resize_emul(sb.ctypes.data + (src.offset(0) if src_offset is None else src_offset), sw, sh, src.row_stride, src.frame_stride,
                       out.ctypes.data + dst.offset(0), dst.width, dst.height, dst.row_stride, dst.frame_stride, dst.n, dst.fmt,
                       code(INTERPS, interp))
    return rc, out


def host_resize_image(L, img, dw, dh, interp):
    """the host core on one contiguous [H, W, C] image (C 1, 3 or 4) -> [dh, dw, C]"""
    img = np.ascontiguousarray(img, np.uint8)
    sh, sw, ch = img.shape
    out = np.zeros((dh, dw, ch), np.uint8)
    fmt = {1: FORMATS["gray"], 3: FORMATS["bgr"], 4: FORMATS["bgra"]}[ch]
    rc = L.resize_emul(img.ctypes.data, sw, sh, sw * ch, sw * sh * ch, out.ctypes.data, dw, dh, dw * ch, dw * dh * ch, 1, fmt, code(INTERPS, interp))
    assert rc == 0, rc
    return out


def host_scale_records(L, recs, counts, src_size, dst_size, pose=False, cam=None):
    """the host core on records [n, stride] under counts [n] -> the records afterwards (slots beyond a count as they were)"""
    recs = np.ascontiguousarray(recs)
    out = recs.copy()
    counts = np.ascontiguousarray(counts, np.int32)
    L.scale_records_emul(recs.ctypes.data, counts.ctypes.data, recs.shape[0], recs.shape[1], src_size[0], src_size[1], dst_size[0], dst_size[1],
                         1 if pose else 0, C.addressof(cam) if cam is not None else None, out.ctypes.data)
    return out


# ---- numpy restatement of the rules (float64 / float32 / int64 as stated; np.rint rounds halves to even) ---------------------------------

def np_scale(s, d):
    return np.float64(1.0) / (np.float64(d) / np.float64(s))


def np_nearest_index(s, d):
    return np.minimum(np.floor(np.arange(d) * np_scale(s, d)).astype(np.int64), s - 1)


def np_linear_taps(s, d):
    """(s0, s1, a0, a1) of every destination index of an axis"""
    f = ((np.arange(d, dtype=np.float64) + 0.5) * np_scale(s, d) - 0.5).astype(np.float32)
    s0 = np.floor(f).astype(np.int64)
    f = f - s0.astype(np.float32)
    assert f.dtype == np.float32
    lo = s0 < 0
    s0[lo], f[lo] = 0, 0
    hi = s0 >= s - 1
    s0[hi], f[hi] = s - 1, 0
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s0, np.minimum(s0 + 1, s - 1), a0, a1


def np_area_table(s, d):
    """per destination index the list of (source index, float32 weight) in table order"""
    scale = np_scale(s, d)
    tab = []
    for i in range(d):
        f1 = np.float64(i) * scale
        f2 = f1 + scale
        cell = min(scale, np.float64(s) - f1)
        s1, s2 = int(np.ceil(f1)), min(int(np.floor(f2)), s - 1)
        s1 = min(s1, s2)
        e = []
        if s1 - f1 > 1e-3:
            e.append((s1 - 1, np.float32((s1 - f1) / cell)))
        e += [(k, np.float32(np.float64(1.0) / cell)) for k in range(s1, s2)]
        if f2 - s2 > 1e-3:
            e.append((s2, np.float32(min(min(f2 - s2, np.float64(1.0)), cell) / cell)))
        tab.append(e)
    return tab


def np_sat_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def np_plan(sw, sh, dw, dh, interp):
    """(kind, kx, ky) of a call"""
    interp = code(INTERPS, interp)
    sx, sy = np_scale(sw, dw), np_scale(sh, dh)
    if interp == 1 and sx == 2.0 and sy == 2.0:
        interp = 2
    if interp < 2:
        return interp, 1, 1
    ix, iy = int(np.rint(sx)), int(np.rint(sy))
    eps = np.finfo(np.float64).eps
    if abs(sx - ix) < eps and abs(sy - iy) < eps:
        return KIND_BOX, ix, iy
    return KIND_TABLE, 1, 1


def np_resize(img, dw, dh, interp):
    """[H, W, C] uint8 -> [dh, dw, C] uint8 by the stated rules"""
    sh, sw, ch = img.shape
    kind, kx, ky = np_plan(sw, sh, dw, dh, interp)
    S = img.astype(np.int64)
    if kind == KIND_NEAREST:
        return img[np_nearest_index(sh, dh)][:, np_nearest_index(sw, dw)].copy()
    if kind == KIND_LINEAR:
        x0, x1, a0, a1 = np_linear_taps(sw, dw)
        y0, y1, b0, b1 = np_linear_taps(sh, dh)
        a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[:, None, None], b1[:, None, None]
        r0 = S[y0][:, x0] * a0 + S[y0][:, x1] * a1
        r1 = S[y1][:, x0] * a0 + S[y1][:, x1] * a1
        assert max(np.abs(r0).max(), np.abs(r1).max()) < 2 ** 31 and (np.abs(b0) * (np.abs(r0) >> 4)).max() < 2 ** 31   # (int32 holds them)
        D = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
        assert D.min() >= 0 and D.max() <= 255
        return D.astype(np.uint8)
    if kind == KIND_BOX:
        assert sw == kx * dw and sh == ky * dh
        total = S.reshape(dh, ky, dw, kx, ch).sum((1, 3))
        if kx == 2 and ky == 2:
            return ((total + 2) >> 2).astype(np.uint8)
        return np_sat_u8(total.astype(np.float32) * np.float32(np.float64(1.0) / np.float64(kx * ky)))
    tx, ty = np_area_table(sw, dw), np_area_table(sh, dh)
    nmax = max(len(e) for e in tx)
    # the x taps padded to one length with weight 0 on a valid index: adding +0.0 changes no float
    xi = np.array([[e[k][0] if k < len(e) else e[-1][0] for e in tx] for k in range(nmax)])
    xw = np.array([[e[k][1] if k < len(e) else np.float32(0) for e in tx] for k in range(nmax)], np.float32)
    F = img.astype(np.float32)
    out = np.zeros((dh, dw, ch), np.uint8)
    for y in range(dh):
        acc = np.zeros((dw, ch), np.float32)
        for sy, beta in ty[y]:
            row = np.zeros((dw, ch), np.float32)
            for k in range(nmax):
                row = row + F[sy, xi[k]] * xw[k][:, None]
            acc = acc + beta * row
        assert acc.dtype == np.float32
        out[y] = np_sat_u8(acc)
    return out


def np_scale_coords(p, s, d):
    """float32 coordinates of an axis s -> d"""
    p = np.asarray(p, np.float32)
    if s == d:
        return p.copy()
    v = ((p.astype(np.float64) + 0.5) * (np.float64(d) / np.float64(s)) - 0.5).astype(np.float32)
    v[np.isnan(v)] = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    return v


def np_scale_squares(sq, src_size, dst_size):
    """[..., 8] float32 squares"""
    sq = np.asarray(sq, np.float32)
    out = sq.copy()
    out[..., 0::2] = np_scale_coords(sq[..., 0::2], src_size[0], dst_size[0])
    out[..., 1::2] = np_scale_coords(sq[..., 1::2], src_size[1], dst_size[1])
    return out


# ---- the chain's scenes ------------------------------------------------------------------------------------------------------------------

CHAIN_SMALL = (640, 480)                 # the size detected at
CHAIN_FULL = (1280, 960)                 # the size of the frames: 2 W x 2 H
# (u, v, side in px, tilt, in-plane angle, tilt axis, template) at full size: sides of 120 px or more, tilts up to 50 degrees, three
# templates -- scenes on which the oracle reads the planted template at both sizes (it takes a 4 x 4 marker of 180 px under 30
# degrees for the 2 x 2 template at either size: such scenes say nothing about resizing)
CHAIN_SPECS = [(860, 600, 240, 30, 60, 120, 2), (700, 500, 300, 30, 60, 120, 1), (640, 480, 340, 50, 130, 250, 0), (300, 300, 128, 30, 60, 10, 0)]


def chain_scenes():
    """one persp_synth scene per spec: a single marker on a 1280 x 960 frame"""
    return [PS.scene("chain", "chain-%d" % i, CHAIN_FULL[0], CHAIN_FULL[1], [(u, v, s, tilt, g, ph, tpl, None)])
            for i, (u, v, s, tilt, g, ph, tpl) in enumerate(CHAIN_SPECS)]


def chain_templates():
    return H.oracle_templates(PS.NAMES)


def best_corner_distance(a, b):
    """the largest corner distance of two squares under the best cyclic shift (a square found at another size may start at
    another corner)"""
    a, b = np.asarray(a, np.float64).reshape(4, 2), np.asarray(b, np.float64).reshape(4, 2)
    return min(np.linalg.norm(np.roll(a, k, axis=0) - b, axis=1).max() for k in range(4))

"""Projective warps for the warp tests (ocvar_hip_warp / ocvar_hip_warp_records / ocvar_hip_board_plane_maps): the host build of
opencv-ar_amd/csrc/warp_core.h (tests/emul/warp_emul.cpp), a numpy restatement of the sampler, the record map and the plane map that
shares no code with it, guarded frames (frame_kit.pix_layout), the maps the CPU and GPU tests share, and the
bird's-eye chain on board_chain's scenes.  Shared by tests/test_warp_cpu.py and tests/test_gpu_warp.py."""
import ctypes as C
import math

import numpy as np

import board_chain as BC
from frame_kit import FORMATS, GUARD, pix_layout
from hostbuild import host_core

FMT_NAMES = {v: k for k, v in FORMATS.items()}
NEAREST, LINEAR = 0, 1
CONSTANT, REPLICATE = 0, 1
INTERPS = {"nearest": NEAREST, "linear": LINEAR}
BORDERS = {"constant": CONSTANT, "replicate": REPLICATE}
INVERSE_MAP, ONE_MAP, POSE = 1, 2, 4
# warp.hip: a workgroup owns a destination tile of WARP_TILE_W x warp_tile_h(bytes per pixel) pixels, a lane 4 consecutive ones; the
# LDS image of a staged tile's source window holds WARP_LDS_DWORDS dwords (warp_core.h; tests/test_warp_cpu.py compares these with
# the core's)
TILE_W, LANE_PX, LDS_DWORDS = 64, 4, 4096
TILE_HS = {1: 64, 3: 32, 4: 32}       # bytes per pixel -> the tile's height
TILE_H = max(TILE_HS.values())         # (the sizes of PLAN_CASES are cut for the taller tile; the shorter one divides it)
# The largest corner error of the bird's-eye chain, measured on the CPU over the CHAIN_SCENES scenes of chain_scenes (DESIGN.md 9n:
# 1.07 px), plus one resampling's worth; not above the 2 px of the undistort chain.
CHAIN_SCENES = 4
CHAIN_MEASURED_PX = 1.07
CHAIN_BAR_PX = min(CHAIN_MEASURED_PX + 1.0, 2.0)
NAN_BITS = 0x7FC00000


def build_emul():
    L = host_core("warp_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.warp_emul.argtypes = [vp, i, i, ll, ll, vp, i, i, ll, ll, i, i, vp, i, i, vp, i, vp]
    L.warp_map_emul.argtypes = [vp, i, vp]
    L.warp_source_emul.argtypes = [vp, i, i, i, vp]
    L.warp_records_emul.argtypes = [vp, vp, i, i, vp, i, vp, vp]
    L.warp_board_plane_maps_emul.argtypes = [vp, i, vp, vp, i, i, vp]
    L.warp_tile_plan_emul.argtypes = [vp, i, i, i, i, i, i, i, i, i, vp]
    L.warp_plan_count_emul.argtypes = [vp, i, i, i, i, i, i, i, i, vp]
    L.warp_patch_reference_emul.argtypes = [vp, i, i, ll, i, vp, i, i, vp, vp]
    L.warp_sincos_emul.argtypes = [C.c_double, vp]
    return L


def maps_array(maps):
    """one map or a list of maps -> contiguous float64 [n, 9]"""
    return np.ascontiguousarray(np.asarray(maps, np.float64).reshape(-1, 9))


def fill_bytes(fill):
    return None if fill is None else np.ascontiguousarray(list(fill) + [0] * (4 - len(fill)), np.uint8)


def dst_layout(src, size, aligned, fill=GUARD, n=None):
    """guarded destination frames of size = (width, height) for the frames of src"""
    return pix_layout(src.n if n is None else n, size[0], size[1], FMT_NAMES[src.fmt], aligned, fill=fill)


def host_warp(L, src, dst, maps, interp=LINEAR, border=CONSTANT, fill=None, flags=0, buf=None):
    """the host core: the frames of src.buf (or buf) -> (return code = frames warped, dst's buffer afterwards, status [n])"""
    sb = np.ascontiguousarray(src.buf if buf is None else buf)
    out = dst.buf.copy()
    m = maps_array(maps)
    assert m.shape[0] == (1 if flags & ONE_MAP else dst.n)
    status = np.full(dst.n, -7, np.int32)
    fb = fill_bytes(fill)
    rc = L.warp_emul(sb.ctypes.data + src.offset(0), src.width, src.height, src.row_stride, src.frame_stride, out.ctypes.data + dst.offset(0),
                     dst.width, dst.height, dst.row_stride, dst.frame_stride, dst.n, dst.fmt, m.ctypes.data, interp, border,
                     None if fb is None else fb.ctypes.data, flags, status.ctypes.data)
    return rc, out, status


def host_warp_image(L, img, m, size, interp=LINEAR, border=CONSTANT, fill=None, flags=0, background=None):
    """the host core on one contiguous [H, W, C] image (C 1, 3 or 4) -> (the warped [size[1], size[0], C] image, status)"""
    img = np.ascontiguousarray(img, np.uint8)
    sh, sw, ch = img.shape
    dw, dh = size
    out = np.zeros((dh, dw, ch), np.uint8) if background is None else np.full((dh, dw, ch), background, np.uint8)
    fmt = {1: FORMATS["gray"], 3: FORMATS["bgr"], 4: FORMATS["bgra"]}[ch]
    mm = maps_array(m)
    status = np.zeros(1, np.int32)
    fb = fill_bytes(fill)
    rc = L.warp_emul(img.ctypes.data, sw, sh, sw * ch, sw * sh * ch, out.ctypes.data, dw, dh, dw * ch, dw * dh * ch, 1, fmt, mm.ctypes.data, interp, border,
                     None if fb is None else fb.ctypes.data, flags, status.ctypes.data)
    assert rc >= 0, rc
    return out, int(status[0])


def host_map(L, m, flags=0):
    """the status rule: (ok, M destination -> source [9])"""
    mm, M = maps_array(m), np.zeros(9)
    ok = L.warp_map_emul(mm.ctypes.data, flags, M.ctypes.data)
    return bool(ok), M


def host_warp_records(L, recs, counts, maps, flags=0, cam=None, out=None):
    """the host core on records [n, stride] under counts [n] -> (return code, the records afterwards: slots beyond a count as they
    were in recs, or in out when given)"""
    recs = np.ascontiguousarray(recs)
    out = recs.copy() if out is None else np.ascontiguousarray(out).copy()
    counts = np.ascontiguousarray(counts, np.int32)
    m = maps_array(maps)
    rc = L.warp_records_emul(recs.ctypes.data, counts.ctypes.data, recs.shape[0], recs.shape[1], m.ctypes.data, flags,
                             C.addressof(cam) if cam is not None else None, out.ctypes.data)
    return rc, out


def host_plane_maps(L, poses, K, rect, size):
    """the host core: BOARD poses (a numpy array of 192-byte records or a list of board_chain.BoardPose) -> maps [n, 9]"""
    if not isinstance(poses, np.ndarray):
        poses = np.frombuffer(b"".join(bytes(p) for p in poses), np.uint8)
    raw = np.ascontiguousarray(poses).view(np.uint8).reshape(-1, 192)
    Kc, rc = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(rect, np.float64)
    out = np.zeros((raw.shape[0], 9))
    L.warp_board_plane_maps_emul(raw.ctypes.data, raw.shape[0], Kc.ctypes.data, rc.ctypes.data, size[0], size[1], out.ctypes.data)
    return out


def plan_counts(L, m, src_size, dst_size, bpp, interp=LINEAR, border=CONSTANT, flags=0):
    """the kernel's tiles of one frame: dict(ok, staged, direct, missed, taps, words)"""
    mm, out = maps_array(m), np.zeros(5, np.int64)
    ok = L.warp_plan_count_emul(mm.ctypes.data, flags, src_size[0], src_size[1], dst_size[0], dst_size[1], bpp, interp, border, out.ctypes.data)
    return dict(ok=ok, staged=int(out[0]), direct=int(out[1]), missed=int(out[2]), taps=int(out[3]), words=int(out[4]))


def board_pose(R, t, status=1):
    p = BC.BoardPose()
    p.rvec[:] = [float(v) for v in BC.rvec_of(np.asarray(R, np.float64))]
    p.tvec[:] = [float(v) for v in t]
    p.status = status
    return p


# ---- the maps the tests share ------------------------------------------------------------------------------------------------------------

def about_centre(src_size, dst_size, scale, degrees=0.0, gx=0.0, gy=0.0):
    """the FORWARD map that turns the source by `degrees` about its centre, scales it by `scale`, adds the perspective terms (gx, gy)
    per source pixel and puts the source's centre on the destination's"""
    (sw, sh), (dw, dh) = src_size, dst_size
    a = math.radians(degrees)
    T0 = np.array([[1, 0, -(sw - 1) / 2], [0, 1, -(sh - 1) / 2], [0, 0, 1.0]])
    A = np.array([[scale * math.cos(a), -scale * math.sin(a), 0], [scale * math.sin(a), scale * math.cos(a), 0], [gx, gy, 1.0]])
    T1 = np.array([[1, 0, (dw - 1) / 2], [0, 1, (dh - 1) / 2], [0, 0, 1.0]])
    return (T1 @ A @ T0).reshape(9)


def shared_maps(src_size, dst_size):
    """name -> (map [9], flags: 0 for a forward map, INVERSE_MAP for a destination -> source one).  Which classes of the tile plan a
    map shows depends on the sizes: the tests ask plan_counts."""
    (sw, sh), (dw, dh) = src_size, dst_size
    return {
        "identity": (np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), 0),
        "shift": (np.array([1, 0, 3, 0, 1, -2, 0, 0, 1.0]), 0),
        "mild": (about_centre(src_size, dst_size, 1.0, 5.0, 2e-5, -1e-5), 0),                        # the benchmark's map
        "magnify": (about_centre(src_size, dst_size, 3.7, -12.0, 1e-4, 2e-4), 0),                    # small windows: staged
        "fit": (np.array([(dw - 1) / max(sw - 1, 1), 0, 0, 0, (dh - 1) / max(sh - 1, 1), 0, 0, 0, 1.0]) if sw > 1 and sh > 1 and dw > 1 and dh > 1
                else np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), 0),                                         # 300 x 200 -> 8 x 8: direct
        # w = 1 - 1.2 x / dw + ..: positive on the left (the source stretched towards the horizon), through 0 at x = dw / 1.2, negative beyond
        "horizon": (np.array([1, 0.1, 0, 0.05, 1, 0, -1.2 / dw, 0.05 / dh, 1.0]), INVERSE_MAP),
        "outside": (np.array([1, 0, 10 * (sw + dw), 0, 1, -7 * (sh + dh), 0, 0, 1.0]), INVERSE_MAP),   # every tap beyond the source
        "tilted": (np.array([0.9, 0.2, 0.1 * sw, -0.15, 1.1, 0.05 * sh, 4e-4, -3e-4, 1.0]), INVERSE_MAP),
    }


# the cases tests/test_warp_cpu.py counts the classes of and tests/test_gpu_warp.py runs on the device: name -> (source size, destination size, map name, classes it must show)
PLAN_CASES = {
    "magnify": ((90, 60), (2 * TILE_W + 1, 2 * TILE_H + 1), "magnify", "staged"),
    "mild": ((200, 120), (2 * TILE_W + 1, 3 * TILE_H + 1), "mild", "staged"),
    "shrink": ((300, 200), (8, 8), "fit", "direct"),
    "horizon": ((90, 60), (2 * TILE_W + 1, 2 * TILE_H + 1), "horizon", "both"),
    "outside": ((90, 60), (TILE_W + 1, TILE_H + 1), "outside", "staged"),
    "tilted": ((150, 100), (3 * TILE_W, 2 * TILE_H), "tilted", "staged"),
}


SKIPPED_MAPS = {
    "nan": np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1.0]),
    "inf": np.array([1, 0, np.inf, 0, 1, 0, 0, 0, 1.0]),
    "singular": np.array([1, 2, 3, 2, 4, 6, 0, 0, 1.0]),
    "zeros": np.zeros(9),
    "overflow": np.array([1e-200, 0, 0, 0, 1e-200, 0, 0, 0, 1e-200]),     # det underflows to 0 / the inverse is not finite
}


# ---- numpy restatement of the rules -------------------------------------------------------------------------------------------------------

def np_invert(m):
    """the adjugate times 1 / det, in float64, or None when the frame is skipped"""
    m = np.asarray(m, np.float64).reshape(9)
    if not np.isfinite(m).all():
        return None
    a, b, c, d, e, f, g, h, i = m
    with np.errstate(all="ignore"):
        det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
        if det == 0 or not np.isfinite(det):
            return None
        s = 1.0 / det
        M = np.array([(e * i - f * h) * s, (c * h - b * i) * s, (b * f - c * e) * s, (f * g - d * i) * s, (a * i - c * g) * s, (c * d - a * f) * s,
                      (d * h - e * g) * s, (b * g - a * h) * s, (a * e - b * d) * s])
    return M if np.isfinite(M).all() else None


def np_warp(img, m, size, interp=LINEAR, border=CONSTANT, fill=None, flags=0, background=0):
    """[H, W, C] uint8 -> ([size[1], size[0], C], status) by the rules of warp_core.h, restated with numpy arrays: positions in
    float64, 1/32-px fixed point rounded to nearest even, 15-bit weights with the exact-position entry (32767, 0, 0, 1)"""
    img = np.asarray(img, np.uint8)
    sh, sw, ch = img.shape
    dw, dh = size
    out = np.full((dh, dw, ch), background, np.uint8)
    m = np.asarray(m, np.float64).reshape(9)
    M = (m if np.isfinite(m).all() else None) if flags & INVERSE_MAP else np_invert(m)
    if M is None:
        return out, 0
    fillv = np.zeros(4, np.int64) if fill is None else np.array(list(fill) + [0] * (4 - len(fill)), np.int64)
    x, y = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    scale = 32.0 if interp == LINEAR else 1.0
    with np.errstate(all="ignore"):
        W = (M[6] * 0 + M[7] * y + M[8]) + M[6] * x
        Wi = np.where(W != 0, scale / np.where(W != 0, W, 1.0), 0.0)
        Xf = ((M[0] * 0 + M[1] * y + M[2]) + M[0] * x) * Wi
        Yf = ((M[3] * 0 + M[4] * y + M[5]) + M[3] * x) * Wi
    fix = lambda v: np.rint(np.clip(np.where(np.isnan(v), -2147483648.0, v), -2147483648.0, 2147483647.0)).astype(np.int64)   # noqa: E731
    X, Y = fix(Xf), fix(Yf)
    assert not np.isnan(Xf).any() and not np.isnan(Yf).any()    # (finite maps give no NaN: 0 * finite, finite / nonzero)

    def tap(ix, iy):
        if border == REPLICATE:
            return img[np.clip(iy, 0, sh - 1), np.clip(ix, 0, sw - 1)].astype(np.int64)
        inside = (ix >= 0) & (ix < sw) & (iy >= 0) & (iy < sh)
        v = img[np.clip(iy, 0, sh - 1), np.clip(ix, 0, sw - 1)].astype(np.int64)
        return np.where(inside[..., None], v, fillv[:ch][None, None, :])

    if interp == NEAREST:
        return tap(X, Y).astype(np.uint8), 1
    ix, iy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
    exact = (fx | fy) == 0
    w00, w11 = np.where(exact, 32767, w00), np.where(exact, 1, w11)
    acc = (tap(ix, iy) * w00[..., None] + tap(ix + 1, iy) * w01[..., None] + tap(ix, iy + 1) * w10[..., None] + tap(ix + 1, iy + 1) * w11[..., None] + 16384) >> 15
    return acc.astype(np.uint8), 1


def np_warp_squares(sq, m):
    """[..., 8] float32 squares through the forward map m: float64, rounded once to float32, NaN as 0x7FC00000; w == 0 or not finite:
    NaN"""
    sq = np.asarray(sq, np.float32)
    m = np.asarray(m, np.float64).reshape(9)
    x, y = sq[..., 0::2].astype(np.float64), sq[..., 1::2].astype(np.float64)
    with np.errstate(all="ignore"):
        w = m[6] * x + m[7] * y + m[8]
        bad = ~np.isfinite(w) | (w == 0)
        ws = np.where(bad, 1.0, w)
        xo = np.where(bad, np.nan, (m[0] * x + m[1] * y + m[2]) / ws).astype(np.float32)
        yo = np.where(bad, np.nan, (m[3] * x + m[4] * y + m[5]) / ws).astype(np.float32)
    out = np.empty_like(sq)
    out[..., 0::2], out[..., 1::2] = xo, yo
    u = out.view(np.uint32)
    u[np.isnan(out)] = NAN_BITS
    return out


def np_plane_map(R, t, K, rect, size):
    """K [r1 r2 t] S in float64 matrices"""
    dw, dh = size
    x0, y0, x1, y1 = rect
    S = np.array([[(x1 - x0) / (dw - 1) if dw > 1 else 0, 0, x0], [0, (y1 - y0) / (dh - 1) if dh > 1 else 0, y0], [0, 0, 1.0]])
    return (np.asarray(K, np.float64).reshape(3, 3) @ np.c_[R[:, 0], R[:, 1], t] @ S).reshape(9)


def apply_map(M, pts):
    """points [n, 2] through the 3 x 3 map M [9], float64"""
    M = np.asarray(M, np.float64).reshape(3, 3)
    p = np.c_[np.asarray(pts, np.float64), np.ones(len(pts))] @ M.T
    return p[:, :2] / p[:, 2:3]


# ---- the bird's-eye chain -----------------------------------------------------------------------------------------------------------------

CHAIN_PX_PER_UNIT = 80          # destination pixels per board unit (a marker side: the scenes show markers 90 .. 160 px wide)
CHAIN_MARGIN = 0.5              # board units around the markers' bounding box


CHAIN_TURN_DEG = 25.0           # the chain's markers are turned in the board's plane (turned_board says why)


def turned_board(template_ids, cols, rows, length, separation, degrees):
    """board_chain.grid_board's layout with every marker turned by `degrees` about its own centre.  A rectangle of the board's plane
    is axis-aligned in board coordinates, so the markers of grid_board stand axis-aligned in every bird's-eye frame -- and on an
    axis-aligned square with perfectly straight edges the reference's polygon approximation puts every corner (2, 1) px along the
    contour, sqrt(5) = 2.24 px off, however exact the rectification is (measured with the true pose).  Turned markers
    show the chain's own error instead of that."""
    a = math.radians(degrees)
    Rm = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    h = length / 2
    out = []
    for k, t in enumerate(template_ids[:cols * rows]):
        c = np.array([(k % cols) * (length + separation) + h, (k // cols) * (length + separation) + h])
        out.append((t, np.array([[-h, -h], [h, -h], [h, h], [-h, h]]) @ Rm.T + c))
    return out


def chain_scenes(n, cam, degrees=CHAIN_TURN_DEG, seed=11, n_templates=12):
    """board_chain.scenes on the turned board: (names, board, [(bgr, truth, R, t)])"""
    import dense_synth as DS
    names = DS.library(n_templates, size=4, seed=23)
    board = turned_board(list(range(n_templates)), 4, 3, 1.0, 0.5, degrees)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        size = 90 + 70 * ((i * 7) % n) / max(n - 1, 1)
        tilt = 50 * ((i * 5) % n) / max(n - 1, 1)
        R, t = BC.random_pose(rng, board, cam.cameraMatrix[0], size, i % 4, tilt, 1920, 1080)
        bgr, truth = BC.render(board, names, cam, R, t)
        out.append((bgr, truth, R, t))
    return names, board, out


def chain_rect(board):
    """(rect, size): the rectangle of the board's plane the chain looks at -- the markers' bounding box grown by CHAIN_MARGIN, y
    running down the picture as it does in the board's own coordinates -- and the destination size at CHAIN_PX_PER_UNIT"""
    pts = np.concatenate([c for _, c in board])
    x0, y0, x1, y1 = pts[:, 0].min() - CHAIN_MARGIN, pts[:, 1].min() - CHAIN_MARGIN, pts[:, 0].max() + CHAIN_MARGIN, pts[:, 1].max() + CHAIN_MARGIN
    size = (int(round((x1 - x0) * CHAIN_PX_PER_UNIT)) + 1, int(round((y1 - y0) * CHAIN_PX_PER_UNIT)) + 1)
    return (x0, y0, x1, y1), size


def board_to_pixels(rect, size, pts):
    """board points [n, 2] -> bird's-eye pixels: the inverse of S"""
    x0, y0, x1, y1 = rect
    p = np.asarray(pts, np.float64)
    return np.c_[(p[:, 0] - x0) * (size[0] - 1) / (x1 - x0), (p[:, 1] - y0) * (size[1] - 1) / (y1 - y0)]


def corner_errors(markers, board, rect, size):
    """per board entry found among the oracle's markers (first with the entry's template and score > 0): the largest distance of its
    four corners, as a cyclic shift of the entry's, from where the layout and rect put them -> {template id: px}"""
    out = {}
    for tid, corners in board:
        found = [m for m in markers if m.templateId == tid and m.score > 0]
        if found:
            out[tid] = BC.truth_shift(np.array(found[0].square), board_to_pixels(rect, size, corners))[1]
    return out

"""Orientation for the orient tests (ocvar_hip_orient / ocvar_hip_orient_records / ocvar_hip_orient_camera): the host build of
opencv-ar_amd/csrc/orient_core.h (tests/emul/orient_emul.cpp), a numpy restatement of the table that shares no code with it
(numpy's own rot90 / slicing / transpose for frames, float64 for coordinates and the camera), guarded frames
(frame_kit.pix_layout) and the single-marker scenes of resize_chain.  Shared by tests/test_orient_cpu.py
and tests/test_gpu_orient.py."""
import ctypes as C

import numpy as np

import helpers as H
from frame_kit import FORMATS, GUARD, MARKER_DTYPE, pix_layout
from hostbuild import host_core
from resize_chain import chain_scenes, chain_templates, CHAIN_FULL  # noqa: F401

ORIENTS = {"identity": 0, "rot90": 1, "rot180": 2, "rot270": 3, "flip_h": 4, "flip_v": 5, "transpose": 6, "transverse": 7}
NAMES = list(ORIENTS)
FMT_NAMES = {v: k for k, v in FORMATS.items()}
TRANSPOSING, MIRRORING = (1, 3, 6, 7), (4, 5, 6, 7)
ROTATIONS = (0, 1, 2, 3)
INVERSE = {0: 0, 1: 3, 2: 2, 3: 1, 4: 4, 5: 5, 6: 6, 7: 7}
# the kernel class of an orientation (orient.hip)
CLASS = {0: "rows kept", 5: "rows kept", 4: "rows reversed", 2: "rows reversed", 1: "transposing", 3: "transposing", 6: "transposing",
         7: "transposing"}
ORIENT_POSE = 1
# orient.hip: a lane of the row kernels owns ORIENT_LANE_PX = 8 destination pixels, a wave 512; the transposing kernel moves tiles
# of ORIENT_TILE = 64 pixels a side, a lane assembling ORIENT_TILE_RUN = 4 destination pixels
LANE_PX, WAVE_PX, TILE, TILE_RUN = 8, 512, 64, 4
ROW_GROUP = 4      # orient_rows(1): at 1 byte per pixel a workgroup of the row kernels takes its span in 4 consecutive rows
# 1, 2, 3, both sides of a lane's run of either kind, both sides of the tile, a third tile
SIDES = sorted({1, 2, 3, 7, 8, 9, 63, 64, 65, 129, TILE_RUN - 1, TILE_RUN, TILE_RUN + 1, LANE_PX - 1, LANE_PX, LANE_PX + 1, TILE - 1, TILE, TILE + 1,
                2 * TILE + 1, ROW_GROUP - 1, ROW_GROUP, ROW_GROUP + 1})
# widths that put both sides of a wave's span of the row kernels, and a second workgroup, into a row
WIDE = [WAVE_PX - 1, WAVE_PX, WAVE_PX + 1]
NAN_BITS = 0x7FC00000


def build_emul():
    L = host_core("orient_emul")
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    L.orient_emul.argtypes = [vp, i, i, ll, ll, vp, ll, ll, i, i, i]
    L.orient_source_index_emul.argtypes = [i, i, i, i, i, vp]
    L.orient_records_emul.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp]
    L.orient_camera_emul.argtypes = [vp, i, vp]
    return L


def code(o):
    return ORIENTS[o] if isinstance(o, str) else int(o)


def oriented_size(size, o):
    return (size[1], size[0]) if code(o) in TRANSPOSING else (size[0], size[1])


def dst_layout(src, o, aligned, fill=GUARD):
    """guarded destination frames for the frames of src under orientation o"""
    dw, dh = oriented_size((src.width, src.height), o)
    return pix_layout(src.n, dw, dh, FMT_NAMES[src.fmt], aligned, fill=fill)


def host_orient(L, src, dst, o, buf=None, src_offset=None, src_size=None):
    """the host core: the frames of src.buf (or buf) -> (return code, dst's buffer afterwards); src_offset / src_size: a source
    rectangle (byte offset of its first pixel, its (width, height)) with src's strides"""
    sb = np.ascontiguousarray(src.buf if buf is None else buf)
    out = dst.buf.copy()
    sw, sh = (src.width, src.height) if src_size is None else src_size
    rc = L.orient_emul(sb.ctypes.data + (src.offset(0) if src_offset is None else src_offset), sw, sh, src.row_stride, src.frame_stride,
                       out.ctypes.data + dst.offset(0), dst.row_stride, dst.frame_stride, dst.n, dst.fmt, code(o))
    return rc, out


def host_orient_image(L, img, o):
    """the host core on one contiguous [H, W, C] image (C 1, 3 or 4) -> the oriented image"""
    img = np.ascontiguousarray(img, np.uint8)
    sh, sw, ch = img.shape
    dw, dh = oriented_size((sw, sh), o)
    out = np.zeros((dh, dw, ch), np.uint8)
    fmt = {1: FORMATS["gray"], 3: FORMATS["bgr"], 4: FORMATS["bgra"]}[ch]
    rc = L.orient_emul(img.ctypes.data, sw, sh, sw * ch, sw * sh * ch, out.ctypes.data, dw * ch, dw * dh * ch, 1, fmt, code(o))
    assert rc == 0, rc
    return out


def host_orient_records(L, recs, counts, src_size, o, pose=False, cam=None, out=None):
    """the host core on records [n, stride] under counts [n] -> (return code, the records afterwards: slots beyond a count as they
    were in recs, or in out when given)"""
    recs = np.ascontiguousarray(recs)
    out = recs.copy() if out is None else np.ascontiguousarray(out).copy()
    counts = np.ascontiguousarray(counts, np.int32)
    rc = L.orient_records_emul(recs.ctypes.data, counts.ctypes.data, recs.shape[0], recs.shape[1], src_size[0], src_size[1], code(o),
                               ORIENT_POSE if pose else 0, C.addressof(cam) if cam is not None else None, out.ctypes.data)
    return rc, out


def host_orient_camera(L, cam, o):
    """the host core on a helpers.Camera -> (return code, the new camera)"""
    out = H.Camera()
    rc = L.orient_camera_emul(C.addressof(cam), code(o), C.addressof(out))
    return rc, out


# ---- numpy restatement of the table --------------------------------------------------------------------------------------------------

def np_orient(a, o):
    """[H, W, C] -> the oriented image, by numpy's own operations (the table's numpy column)"""
    o = code(o)
    return [lambda: a, lambda: np.rot90(a, -1), lambda: np.rot90(a, 2), lambda: np.rot90(a, 1), lambda: a[:, ::-1], lambda: a[::-1],
            lambda: a.transpose(1, 0, 2), lambda: np.rot90(a, 2).transpose(1, 0, 2)][o]().copy()


def np_orient_points(p, size, o):
    """[..., 2] float64 points (x, y) of a frame of size = (W, H) -> where they go, float64"""
    p = np.asarray(p, np.float64)
    W, Hh = np.float64(size[0]), np.float64(size[1])
    x, y = p[..., 0], p[..., 1]
    xo, yo = [(x, y), (Hh - 1 - y, x), (W - 1 - x, Hh - 1 - y), (y, W - 1 - x), (W - 1 - x, y), (x, Hh - 1 - y), (y, x), (Hh - 1 - y, W - 1 - x)][code(o)]
    return np.stack([xo, yo], axis=-1)


def np_orient_squares(sq, size, o):
    """[..., 8] float32 squares: float64 through the table, rounded to float32, a NaN as 0x7FC00000; a coordinate the table passes
    on is the same float32, bit for bit"""
    sq = np.asarray(sq, np.float32)
    W, Hh = size
    x, y = sq[..., 0::2], sq[..., 1::2]

    def rev(extent, v):
        r = (np.float64(extent - 1) - v.astype(np.float64)).astype(np.float32)
        r[np.isnan(r)] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
        return r

    xo, yo = [(x, y), (rev(Hh, y), x), (rev(W, x), rev(Hh, y)), (y, rev(W, x)), (rev(W, x), y), (x, rev(Hh, y)), (y, x), (rev(Hh, y), rev(W, x))][code(o)]
    out = np.empty_like(sq)
    out[..., 0::2], out[..., 1::2] = xo, yo
    return out


TANGENTIAL = {0: lambda p1, p2: (p1, p2), 1: lambda p1, p2: (p2, -p1), 2: lambda p1, p2: (-p1, -p2), 3: lambda p1, p2: (-p2, p1),
              4: lambda p1, p2: (p1, -p2), 5: lambda p1, p2: (-p1, p2), 6: lambda p1, p2: (p2, p1), 7: lambda p1, p2: (-p2, -p1)}


def np_gl_projection(width, height, K):
    """cvarCameraProjection(glstyle = 0), transposed as cvarReadCamera stores it: 16 doubles"""
    near, far = 0.1, 5000.0
    p = np.zeros((4, 4))
    p[0, 0] = 2.0 * K[0, 0] / width
    p[1, 1] = 2.0 * K[1, 1] / height
    p[0, 2] = 2.0 * (K[0, 2] / width) - 1.0
    p[1, 2] = 2.0 * (K[1, 2] / height) - 1.0
    p[2, 2] = -(far + near) / (far - near)
    p[2, 3] = -2.0 * far * near / (far - near)
    p[3, 2] = -1
    return p.T.reshape(-1)


def np_orient_camera(cam, o):
    """(width, height, K [3, 3], dist [5], glProjection [16]) of the oriented camera, float64"""
    o = code(o)
    K = np.array(list(cam.cameraMatrix), np.float64).reshape(3, 3)
    d = np.array(list(cam.distCoeffs), np.float64)
    w, h = oriented_size((cam.width, cam.height), o)
    K2 = K.copy()
    if o in TRANSPOSING:
        K2[0, 0], K2[1, 1] = K[1, 1], K[0, 0]
    K2[0, 2], K2[1, 2] = np_orient_points([K[0, 2], K[1, 2]], (cam.width, cam.height), o)
    d2 = d.copy()
    d2[2], d2[3] = TANGENTIAL[o](d[2], d[3])
    return w, h, K2, d2, np_gl_projection(w, h, K2)


def np_distort(K, d, n):
    """normalised points [..., 2] -> pixels under the five-coefficient model, float64"""
    x, y = n[..., 0], n[..., 1]
    k1, k2, p1, p2, k3 = d
    r2 = x * x + y * y
    cd = 1 + (k1 + (k2 + k3 * r2) * r2) * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], axis=-1)


# the turn of the normalised image plane (and of the camera frame about the optical axis) under the rotations: n' = Z n
PLANE_TURN = {0: np.array([[1.0, 0], [0, 1]]), 1: np.array([[0.0, -1], [1, 0]]), 2: np.array([[-1.0, 0], [0, -1]]), 3: np.array([[0.0, 1], [-1, 0]]),
              4: np.array([[-1.0, 0], [0, 1]]), 5: np.array([[1.0, 0], [0, -1]]), 6: np.array([[0.0, 1], [1, 0]]), 7: np.array([[0.0, -1], [-1, 0]])}


def turned_glmatrix(gl, o):
    """the 16 doubles of a pose turned about the optical axis with the picture (rotations only): Z M, M the matrix glMatrix holds
    column by column"""
    M = np.asarray(gl, np.float64).reshape(4, 4).T
    Z = np.eye(4)
    Z[:2, :2] = PLANE_TURN[code(o)]
    return (Z @ M).T.reshape(-1)


def gl_reprojection(gl, cam, ratio):
    """the pixels [4, 2] the pose in glMatrix puts the marker's model corners (cvarSquareInit with `ratio`) at under cam: glMatrix
    holds F R F and F t, F = diag(1, 1, -1), column by column (pose_core.h: gl_from_pose)"""
    M = np.asarray(gl, np.float64).reshape(4, 4).T
    F = np.diag([1.0, 1.0, -1.0])
    R, t = F @ M[:3, :3] @ F, F @ M[:3, 3]
    obj = np.array([[-ratio, -1, 0], [ratio, -1, 0], [ratio, 1, 0], [-ratio, 1, 0]], np.float64)
    X = obj @ R.T + t
    K = np.array(list(cam.cameraMatrix), np.float64).reshape(3, 3)
    return np_distort(K, np.array(list(cam.distCoeffs), np.float64), X[:, :2] / X[:, 2:3])


def records_of(markers, slots=None):
    """oracle markers (helpers.Marker) -> [1, slots] records"""
    recs = np.zeros((1, max(len(markers), 1) if slots is None else slots), MARKER_DTYPE)
    for k, m in enumerate(markers):
        recs[0, k] = np.frombuffer(bytes(m), MARKER_DTYPE)[0]
    return recs

"""Patches for the patch tests (ocvar_hip_patches / ocvar_hip_patches_records): the host build of
opencv-ar_amd/csrc/patch_core.h (tests/emul/patch_emul.cpp), guarded patch buffers, the random quads of the oracle parity test
and the oracle chain (orc_get_perspective_transform + orc_warp_perspective_gray per channel plane).  Frames, records and guard
bytes are frame_kit's.  Shared by tests/test_patches_cpu.py and tests/test_gpu_patches.py."""
import ctypes as C

import numpy as np

import helpers as H
from frame_kit import GUARD, LEAD
from helpers import P
from hostbuild import host_core

MAX_PATCH_SIDE, FLIP_ROWS, MATCHED_ONLY = 256, 1, 2
STATUS_FILL = -7   # what a status array holds before a call: every entry must be written
SIZES = [(2, 2), (3, 5), (16, 16), (63, 17), (64, 64), (65, 33), (256, 2), (256, 256)]   # (patch_w, patch_h)


def build_emul():
    L = host_core("patch_emul")
    L.patch_extract_frame_emul.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.patch_map32_emul.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


class Patches:
    """the patch block [n, slots, ph, pw, bpp] inside one guarded byte buffer: `lead` guard bytes in front (an odd lead puts the
    block at an odd address), LEAD behind, and the block itself filled with GUARD too -- a slot that is not written is guard"""

    def __init__(self, n, slots, pw, ph, bpp, lead=LEAD):
        self.n, self.slots, self.pw, self.ph, self.bpp, self.lead = n, slots, pw, ph, bpp, lead
        self.slot_bytes = pw * ph * bpp
        self.buf = np.full(lead + n * slots * self.slot_bytes + LEAD, GUARD, np.uint8)

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[self.lead:self.lead + self.n * self.slots * self.slot_bytes].reshape(self.n, self.slots, self.ph, self.pw, self.bpp)


def host_patches(L, frames, recs, counts, pw, ph, flags=0, per_frame=None, lead=LEAD, buf=None):
    """the host core on frames.buf (or buf): recs [n, stride >= per_frame] records, counts [n] -> (Patches, its filled buffer,
    status [n, per_frame])"""
    src = frames.buf if buf is None else buf
    recs = np.ascontiguousarray(recs)
    slots = recs.shape[1] if per_frame is None else per_frame
    assert recs.shape[1] >= slots
    pt = Patches(frames.n, slots, pw, ph, frames.bpp, lead)
    out = pt.buf.copy()
    status = np.full((frames.n, slots), STATUS_FILL, np.int32)
    for f in range(frames.n):
        L.patch_extract_frame_emul(src.ctypes.data + frames.offset(f), frames.width, frames.height, frames.row_stride, frames.fmt,
                                   recs[f].ctypes.data, int(counts[f]), slots, out.ctypes.data + lead + f * slots * pt.slot_bytes,
                                   pw, ph, flags, status[f].ctypes.data)
    return pt, out, status


def random_quads(rng, n, W, Hh):
    """n quads [n, 4, 2] float32: sides of 4 .. 200 px, turned and sheared at random, centres up to 5 px beyond the W x Hh frame,
    every third one rounded to integers"""
    sq = np.zeros((n, 4, 2), np.float64)
    unit = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
    for k in range(n):
        sx, sy = rng.uniform(4, 200, 2)
        a, sh = rng.uniform(0, 2 * np.pi), rng.uniform(-0.5, 0.5)
        A = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ np.array([[1, sh], [0, 1]]) @ np.diag([sx, sy])
        c = np.array([rng.uniform(-5, W + 5), rng.uniform(-5, Hh + 5)])
        sq[k] = c + unit @ A.T + rng.uniform(-0.06, 0.06, (4, 2)) * min(sx, sy)   # (the last term: a perspective)
        if k % 3 == 2:
            sq[k] = np.rint(sq[k])
    return sq.astype(np.float32)


def dst_square(pw, ph):
    """cvarSquare(pw, ph, ccw = 0)"""
    return np.array([0, 0, pw - 1, 0, pw - 1, ph - 1, 0, ph - 1], np.float32)


def core_map32(L, square, pw, ph):
    m = np.zeros(9, np.float32)
    sq = np.ascontiguousarray(square, np.float32).reshape(8)
    return m if L.patch_map32_emul(P(sq), pw, ph, P(m)) else None


def oracle_map32(square, pw, ph):
    m = np.zeros(9, np.float32)
    sq, dst = np.ascontiguousarray(square, np.float32).reshape(8), dst_square(pw, ph)
    H.oracle().orc_get_perspective_transform(P(sq), P(dst), P(m))
    return m


def oracle_warp(planes, m32, pw, ph):
    """the oracle's warp of every channel plane (contiguous [H, W] uint8 arrays) under map m32 -> [ph, pw, channels]"""
    out = np.zeros((ph, pw, len(planes)), np.uint8)
    m = np.ascontiguousarray(m32, np.float32)
    for c, pl in enumerate(planes):
        dst = np.zeros((ph, pw), np.uint8)
        H.oracle().orc_warp_perspective_gray(P(pl), pl.shape[1], pl.shape[0], pl.shape[1], P(m), P(dst), pw, ph)
        out[..., c] = dst
    return out


def planes_of(frames, f, buf=None):
    v = frames.view(f, buf)
    return [np.ascontiguousarray(v[..., c]) for c in range(frames.bpp)]

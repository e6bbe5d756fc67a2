"""Frames at the size limits of the C ABI (contexts of up to 32767 pixels each way) for tests/test_gpu_geometry_limits.py and
tests/test_geometry_limits_cpu.py: long thin frames with synthetic scenes at the origin, the centre and the far corner, frames
of random blocks one strip or one chunk wide, one very large marker, and small frames whose markers lie in the bottom rows."""
import ctypes as C

import numpy as np

import helpers as H

FAR = 32767                      # the largest width / height ocvar_hip_create admits
CANVAS = 220
# one template set per pasted scene, so that the stateless elimination (one marker per template) keeps markers of all of them
SCENE_TEMPLATES = [["2x2-01", "3x3-01", "4x4-01"], ["5x5-s1", "6x6-s1", "7x7-s1"], ["8x8-s1", "8x8-neg", "8x8-corners"]]
LIBRARY = [n for s in SCENE_TEMPLATES for n in s]
SCENE_FRAMES = (3, 49, 42)       # synthetic frame index of each scene
CUT_FRAME = 2                    # and of the strip of markers the far edge cuts


def pinhole_camera(w, h):
    """fx = fy = max(w, h), principal point at the centre, no distortion.  (cvarCameraScale would stretch the 4:3 default to the
    frame's 55:1, where the planar pose fit has no well-defined minimum: DESIGN.md section 5.)"""
    cam = H.Camera()
    H.oracle().orc_camera_default(C.byref(cam))
    cam.width, cam.height = w, h
    f = float(max(w, h))
    cam.cameraMatrix[:] = [f, 0.0, w / 2.0, 0.0, f, h / 2.0, 0.0, 0.0, 1.0]
    for i in range(5):
        cam.distCoeffs[i] = 0.0
    H.oracle().orc_camera_scale(C.byref(cam), w, h)   # (ratio 1: recomputes glProjection for this matrix)
    return cam


def _scene(w, h, frame, names, **over):
    cfg = H.synth_config(2, width=w, height=h, **over)
    return H.synth_frame(cfg, frame, names)


def long_frame(tall):
    """A 32767 x 600 frame (600 x 32767 when tall) on a flat canvas: three 640 x 480 (480 x 640) scenes at the origin, at the
    centre with an even offset and flush with the far corner, and a strip of markers shifted so that the far edge cuts through
    the middle of its last marker.  Returns (frame, regions): regions[name] = (x0, y0, x1, y1) of each paste inside the frame."""
    W, Hh = (600, FAR) if tall else (FAR, 600)
    sw, sh = (480, 640) if tall else (640, 480)
    frame = np.full((Hh, W, 3), CANVAS, np.uint8)
    at = [(0, 0), (((W - sw) // 2) & ~1, ((Hh - sh) // 2) & ~1), (W - sw, Hh - sh)]
    regions = {}
    for k, ((x0, y0), names, idx) in enumerate(zip(at, SCENE_TEMPLATES, SCENE_FRAMES)):
        img, _ = _scene(sw, sh, idx, names)
        frame[y0:y0 + sh, x0:x0 + sw] = img
        regions[("origin", "centre", "far")[k]] = (x0, y0, x0 + sw, y0 + sh)
    # the strip lies in the 120 columns (rows) the far scene leaves free beside it; its last marker's centre goes onto the far edge
    cw, ch = (120, 480) if tall else (480, 120)
    img, truth = _scene(cw, ch, CUT_FRAME, SCENE_TEMPLATES[0], grid_x=1 if tall else 3, grid_y=3 if tall else 1, side_min=60, side_max=80)
    c = truth[-1]["corner"].mean(0)
    if tall:
        x0, y0 = 0, Hh - int(c[1])
        frame[y0:Hh, x0:x0 + cw] = img[:Hh - y0]
        regions["cut"] = (x0, y0, x0 + cw, Hh)
    else:
        x0, y0 = W - int(c[0]), 0
        frame[y0:y0 + ch, x0:W] = img[:, :W - x0]
        regions["cut"] = (x0, y0, W, y0 + ch)
    return frame, regions


def inside(square, region):
    """all four corners of a record's square (8 floats) inside region (x0, y0, x1, y1)"""
    q = np.asarray(square, np.float64).reshape(4, 2)
    x0, y0, x1, y1 = region
    return bool((q[:, 0] >= x0).all() and (q[:, 0] < x1).all() and (q[:, 1] >= y0).all() and (q[:, 1] < y1).all())


def block_frame(w, h, seed):
    """random 4 x 4 blocks of black and white (no marker fits a frame 16 or 33 pixels thin; every border rule is at work)"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4, 1), np.uint8) * 255
    return np.ascontiguousarray(np.kron(cells, np.ones((4, 4, 3), np.uint8))[:h, :w])


def big_marker_frame(size=4096, side=2500.0, degrees=20.0, name="4x4-01"):
    """a grey size x size frame with ONE marker `side` pixels on its side, turned by `degrees` about the frame's centre (template
    cells sampled at the nearest cell; canvas elsewhere)"""
    tpl = H.template_pixels()[name][0]
    n = tpl.shape[0]
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float32)
    t = np.float32(np.deg2rad(degrees))
    dx, dy = xs - np.float32(size / 2.0), ys - np.float32(size / 2.0)
    u = (np.cos(t) * dx + np.sin(t) * dy) / np.float32(side) + np.float32(0.5)
    v = (-np.sin(t) * dx + np.cos(t) * dy) / np.float32(side) + np.float32(0.5)
    ok = (u >= 0) & (u < 1) & (v >= 0) & (v < 1)
    iu = np.clip((u * n).astype(np.int32), 0, n - 1)
    iv = np.clip((v * n).astype(np.int32), 0, n - 1)
    cell = tpl[iv, iu]
    return np.where(ok, np.where(cell > 0, np.uint8(235), np.uint8(20)), np.uint8(CANVAS)).astype(np.uint8)


def bottom_rows_frame(frame=0):
    """a 320 x 240 BGR frame on a flat canvas whose three markers all lie in the bottom 100 rows"""
    img, truth = _scene(320, 100, frame, SCENE_TEMPLATES[0], grid_x=3, grid_y=1, side_min=50, side_max=64)
    out = np.full((240, 320, 3), CANVAS, np.uint8)
    out[140:] = img
    return out, [t["corner"] + [0, 140] for t in truth]

"""Synthetic frames with hundreds to thousands of markers (tests/test_gpu_dense.py, tools/dense_scaling.py): a library of
distinct random code grids, one template per planted marker, upright markers on a dense grid."""
import ctypes as C

import numpy as np

import helpers as H


def library(k, size=4, seed=7):
    """k templates of size x size random cells, no two sharing a code in any rotation and none rotationally symmetric"""
    rng = np.random.default_rng(seed)
    seen, names = set(), []
    while len(names) < k:
        g = rng.integers(0, 2, (size, size))
        rots = [tuple(np.rot90(g, r).flatten()) for r in range(4)]
        if len(set(rots)) < 4 or any(r in seen for r in rots):
            continue
        seen.update(rots)
        name = f"dense-{size}-{seed}-{len(names)}"
        H.register_template(name, g)
        names.append(name)
    return names


def config(width, height, grid_x, grid_y, side=50):
    return H.synth_config(3, width=width, height=height, grid_x=grid_x, grid_y=grid_y, side_min=side - 2, side_max=side + 2,
                          rot_mode=2, corner_jitter_pct=0, occlude_pct=0, textured=0)


def frame(cfg, index, names):
    """bgr frame [H, W, 3] with grid_x * grid_y markers (marker n carries template (n + index) % len(names))"""
    tp = H.template_pixels()
    arrs = [np.ascontiguousarray(tp[n][0]) for n in names]
    st = (H.SynthTemplate * len(arrs))()
    for i, a in enumerate(arrs):
        st[i].pixels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        st[i].h, st[i].w = a.shape
    bgr = np.zeros((cfg.height, cfg.width, 3), np.uint8)
    truth = (H.SynthMarker * (cfg.grid_x * cfg.grid_y + 1))()
    H.synth_lib().ocvar_synth_frame(C.byref(cfg), index, st, len(arrs), H.P(bgr), cfg.width * 3, truth, len(truth))
    return bgr


def oracle_squares(gray, max_quads=20000):
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    q = np.zeros(8 * max_quads, np.int32)
    n = H.oracle().orc_find_squares(H.P(g), w, h, w, H.P(q), max_quads)
    assert 0 <= n < max_quads
    return q[:8 * n].reshape(n, 4, 2)


# ---- frames with an exact number of squares (tests/test_gpu_dense_limits.py) ----
# A dark 28 px square on a light ground is one frame-pass square of the oracle (contour area 27^2 > 500); squares sit on a
# 40 px grid, row by row, and a frame is the smallest of FRAME_SIZES whose grid holds them.
FRAME_SIZES = [(640, 480), (1920, 1080), (3840, 2160), (7680, 4320)]
PITCH, SIDE, GROUND, INK = 40, 28, 200, 40


def square_slots(w, h, margin=20, top=0):
    """top-left corners of the grid's squares in a w x h frame, row by row, below row `top`"""
    return [(x, y) for y in range(top + margin, h - SIDE - margin, PITCH) for x in range(margin, w - SIDE - margin, PITCH)]


def frame_size_for(n):
    for w, h in FRAME_SIZES:
        if len(square_slots(w, h)) >= n:
            return w, h
    raise ValueError(f"no frame size holds {n} squares")


def squares_frame(n, width=None, height=None, margin=20, marker_strip=None):
    """grey frame [H, W] whose oracle frame-pass square count is exactly n: the first n squares of the grid (under
    `marker_strip`, a grey image pasted at the top-left corner, when given: the grid fills up what the strip lacks)"""
    if width is None:
        width, height = frame_size_for(n)
    g = np.full((height, width), GROUND, np.uint8)
    top, have = 0, 0
    if marker_strip is not None:
        g[:, :] = marker_strip[0, 0]
        g[:marker_strip.shape[0], :marker_strip.shape[1]] = marker_strip
        top, have = marker_strip.shape[0], strip_squares(marker_strip, width, height)
    slots = square_slots(width, height, margin, top)
    assert 0 <= n - have <= len(slots), (n, have, len(slots))
    for x, y in slots[:n - have]:
        g[y:y + SIDE, x:x + SIDE] = INK
    got = len(oracle_squares(g))
    assert got == n, (n, got)
    return g


def strip_squares(strip, width, height):
    """oracle squares of a width x height frame that holds only the strip (squares_frame: at its top-left corner)"""
    g = np.full((height, width), strip[0, 0], np.uint8)
    g[:strip.shape[0], :strip.shape[1]] = strip
    return len(oracle_squares(g))


def marker_strip(k, names, width=None, side=50):
    """grey strip [100, width] with k upright markers in a row (templates names[0..k)), cut from a frame of the generator"""
    width = width or 100 * max(k, 1)
    cfg = config(width, 100, max(k, 1), 1, side=side)
    return np.ascontiguousarray(frame(cfg, 0, names[:max(k, 1)])[:, :, 0])


def marker_frame(k, names, width=1920, height=1080):
    """bgr frame with k upright markers, one template each (names[0..k)), on a grid of gx x gy = k cells (k = 0: no marker)"""
    if k == 0:
        g = np.full((height, width, 3), GROUND, np.uint8)
        return g
    gx = next(d for d in range(int(np.ceil(np.sqrt(k))), k + 1) if k % d == 0 and k // d <= 9 and d <= 16)
    return frame(config(width, height, gx, k // gx), 0, names[:k])


def concentric_frame(width, height, sides=(120, 96, 72, 48), pitch=150):
    """grey frame of concentric square targets (dark and light rings): every ring border is a square, and the crops of one
    target's squares cover each other"""
    g = np.full((height, width), GROUND, np.uint8)
    big = sides[0]
    for y in range(20, height - big - 20, pitch):
        for x in range(20, width - big - 20, pitch):
            for r, s in enumerate(sides):
                o = (big - s) // 2
                g[y + o:y + o + s, x + o:x + o + s] = INK if r % 2 == 0 else GROUND
    return g

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

"""Scenes for tests/test_gpu_ring_batches.py: batches of 320 x 240 frames whose crop pass has exactly N ROIs, for the group sizes of
follow.hip::ring_quads_kernel<true> (64 consecutive ROIs per wave: a partial group, a full one, a group that spills).  A frame is a
flat light field with dark squares of 30 px; the square finder keeps one quad of each, so each gives one crop of 41 x 41 (the
quad's box and 5 px on each side, decode_core.h::crop_rect), whose own frame border -- the ring of pixels next to cvFindContours'
zeroed frame -- lies in the light field: all set in the crop's binary image.  Every third square has one dark pixel 5 px to its
left, which the crop's binarise turns into exactly one cleared pixel of the ring.  ring_kinds reads both facts from the oracle."""
import numpy as np

import helpers as H
import work_cut_scenes as S

W, HH = 320, 240
SIDE, PITCH, X0, Y0 = 30, 48, 20, 14           # 6 x 5 squares at most in a frame
PER_FRAME = 24                                  # squares of a full frame (the first four rows of six)
COUNTS = (1, 63, 64, 65, 130)                   # crop ROIs of a batch
MIN_FRAMES = 9                                  # the ring kernels run in batches of more than 8 frames


def holed(k):
    """whether square k of a batch (counted through its frames) has the dot that opens its crop's ring"""
    return k % 3 == 2


def frame_of(first, count):
    """BGR frame with squares first .. first + count - 1 of the batch, count <= PER_FRAME"""
    g = np.full((HH, W), 235, np.uint8)
    for j in range(count):
        x, y = X0 + PITCH * (j % 6), Y0 + PITCH * (j // 6)
        g[y:y + SIDE, x:x + SIDE] = 20
        if holed(first + j):
            g[y + 12, x - 5] = 20
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def batch_of(n_rois):
    """(frames [n, 240, 320, 3], squares per frame) of the batch with n_rois crops: full frames first, then empty ones up to 9"""
    per = []
    left = n_rois
    while left > 0:
        per.append(min(left, PER_FRAME))
        left -= per[-1]
    per += [0] * max(0, MIN_FRAMES - len(per))
    first = np.concatenate([[0], np.cumsum(per)[:-1]]).astype(int)
    return np.stack([frame_of(int(f), c) for f, c in zip(first, per)]), per


def ring_kinds(frame_bgr, grey):
    """the crops of a frame as the oracle gives them, [(x0, y0, w, h, pixels of the ring that are not set)]: its frame-pass quads,
    their crop rectangles, and the oracle's binary image of each crop of the grey plane"""
    out = []
    for _, x0, y0, w, h in S.crop_rois(H.oracle_find_squares(grey), frame_bgr.shape[1], frame_bgr.shape[0]):
        b = H.oracle_binarise(grey[y0:y0 + h, x0:x0 + w]) > 0
        sh, sw = b.shape
        assert sw >= 8 and sh >= 8
        ring = np.concatenate([b[1, 1:sw - 1], b[sh - 2, 1:sw - 1], b[1:sh - 1, 1], b[1:sh - 1, sw - 2]])
        out.append((x0, y0, w, h, int((~ring).sum())))
    return out

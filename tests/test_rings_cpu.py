"""CPU tests of the scenes of tests/ring_scenes.py, from the oracle alone: every scene that tests/test_gpu_rings.py runs through
follow.hip::ring_quads_kernel holds the rings it names -- every listed hole position of a frame's ring, crops of every parity and
of more than 256 ring items with every kind of hole, the batches that take the grid-stride loops a second time --, and of the
fact that the rectangle the kernel approximates for a clean ring is never a quad.  (A frame here has three equal channels, and the
oracle's grey of b = g = r = v is v: (1868 + 9617 + 4899) v + 8192 >> 14.  So the grey plane is the drawn one.)"""
import numpy as np
import pytest

import dense_synth as D
import helpers as H
import ring_batch_scenes as B
import ring_scenes as R
import work_cut_scenes as S
from helpers import P


def test_grey_of_equal_channels_is_the_channel():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    grey = H.oracle_registration(R.bgr(g), H.oracle_templates(), H.oracle_camera(16, 16))[2]
    assert np.array_equal(grey[..., 0], g)


# (sw-2) & 15, (sh-2) % 14 or None where the issue does not fix it, trips of the kernel's base loop
FRAME_TABLE = {(98, 67): (0, None, 1), (320, 240): (14, 0, 2), (96, 520): (14, 0, 3), (34, 18): (0, None, 1)}


@pytest.mark.parametrize("size", sorted(FRAME_TABLE))
def test_frame_scenes_reach_every_target(size):
    W, Hh = size
    sw, sh = W & ~1, Hh & ~1
    col_res, row_res, trips = FRAME_TABLE[size]
    tiles, items = R.ring_items(sw, sh)
    assert (sw - 2) & 15 == col_res and (row_res is None or (sh - 2) % 14 == row_res) and (items + 255) // 256 == trips, (tiles, items)
    if size != (34, 18):
        assert items == {(98, 67): 78, (320, 240): 278, (96, 520): 530}[size]
    # the issue's list, spelt out again: every pixel of it must be a target
    last0 = max(((sw - 2) >> 4) << 4, 1)
    want = {(1, 1), (sw - 2, 1), (1, sh - 2), (sw - 2, sh - 2)}
    want |= {(x, y) for x in (2, 15, 16, 17, last0, sw - 2) for y in (1, sh - 2)}
    want |= {(x, y) for x in (1, sw - 2) for y in (2, 13, 14, 15, sh - 3) if y < sh - 2}
    want |= {(x, 1 + i - 2 * tiles) for x in (1, sw - 2) for i in (63, 64, 255, 256) if 2 * tiles < i < items - 1}
    frames, names, where = R.frame_scene(W, Hh)
    assert len(frames) >= R.MIN_FRAMES and names[0] == "clean" and want <= set(where[1:]), want - set(where[1:])
    assert "top_x15_alone" in names   # (the one hole that only the row mask's highest column sees)
    if size == (320, 240):
        assert {R.column_item(sw, sh, y) for x, y in where[1:] if x == 1} >= {63, 64, 255, 256}
    if size == (96, 520):
        assert {R.column_item(sw, sh, y) for x, y in where[1:] if x == sw - 2} >= {63, 64, 255, 256, 511, 512}
    for g, name, p in zip(frames, names, where):
        b = H.oracle_binarise(g)
        assert b.shape == (sh, sw)
        holes = R.cleared(b)
        if p is None:
            assert not holes and R.rule(b) == 1, (size, holes)
        else:
            assert R.dot_reaches(holes, p) and R.rule(b) == 0 and (holes == [p] or not name.endswith("_alone")), (size, name, p, holes)
        if R.FRAME_SIZES[size]:
            assert len(H.oracle_find_squares(g)) >= len(R.FRAME_SIZES[size]), (size, name)   # (the frame has end results to compare)


def test_crop_scene_mixes_shapes_parities_and_holes():
    frames, plan = R.crop_scene()
    assert 9 <= len(frames) <= 12 and frames.shape[1:] == (R.CH, R.CW)
    assert all(r is not None for r in R.edge_rects().values()), R.edge_rects()   # a crop clipped by each of the four frame edges
    triples, parities, reached, sides = set(), set(), set(), set()
    n_clean = n_holed = n_rois = 0
    tall = []
    for g, rows in zip(frames, plan):
        rings = {c[:4]: c[4] for c in R.crop_rings(g)}
        assert sorted(rings) == sorted(roi[1:] for roi, _, _ in rows)   # (the dots change no quad of the frame pass)
        n_rois += len(rings)
        for roi, kind, target in rows:
            _, x0, y0, w, h = roi
            sw, sh = w & ~1, h & ~1
            assert sw >= 8 and sh >= 8
            holes = rings[roi[1:]]
            triples.add((R.plane_stride(sw), sh, sw))
            parities.add((w & 1, h & 1))
            sides |= {s for s in ("left", "top", "right", "bottom") if R.clipped(s, roi)}
            n_clean += not holes
            n_holed += bool(holes)
            if kind is not None and (holes == [target] if kind.endswith("_alone") else R.dot_reaches(holes, target)):
                reached.add(kind)
            if R.ring_items(sw, sh)[1] > 256:
                tall.append((sw, sh, holes))
    assert n_rois > 128 and n_rois == n_clean + n_holed
    assert len(triples) >= 5 and parities == {(0, 0), (0, 1), (1, 0), (1, 1)}, (triples, parities)
    assert 4 * n_clean >= n_rois and 4 * n_holed >= n_rois, (n_clean, n_holed)
    assert reached == set(R.KIND_NAMES), set(R.KIND_NAMES) - reached
    assert sides == {"left", "top", "right", "bottom"}, sides
    # the crop of more than 256 items: clean in some frame, and in some frame holed in items of the second trip alone
    assert len(tall) == len(frames) and any(not holes for _, _, holes in tall)
    assert any(holes and all(1 < y < sh - 2 and R.column_item(sw, sh, y) >= 256 for _, y in holes) for sw, sh, holes in tall), tall


def test_stride_scene_takes_the_frames_loop_twice():
    frames, index = R.stride_scene()
    assert len(index) == R.STRIDE_FRAMES > 4096 and frames.shape[1:] == (R.STRIDE_H, R.STRIDE_W) and len(frames) <= 32
    verdict = np.array([R.rule(H.oracle_binarise(g)) for g in frames])
    assert verdict[0] == 1 and not verdict[1:].any()
    assert all((verdict[index[f]] == 0) == (f % 3 == 2) for f in range(len(index)))
    assert set(index[4096:]) >= {0, int(index[4097])} and verdict[index[4097]] == 0   # (both kinds in the second trip)
    assert set(index.tolist()) == set(range(len(frames)))


def test_dense_scene_takes_the_crops_loop_twice():
    frames, index = R.dense_scene()
    assert len(index) == R.DENSE_FRAMES and frames.shape[1:] == (R.DENSE_H, R.DENSE_W)
    per_frame = []
    for g in frames:
        quads = D.oracle_squares(g)
        assert len(quads) <= R.DENSE_QUADS
        rois = S.crop_rois(quads, R.DENSE_W, R.DENSE_H)
        holed = sum(bool(R.cleared(H.oracle_binarise(g[y0:y0 + h, x0:x0 + w]))) for _, x0, y0, w, h in rois)
        assert 6 * holed >= len(rois) and 2 * holed <= len(rois), (holed, len(rois))   # every fifth square, and no more than half
        per_frame.append(len(rois))
    assert sum(per_frame[i] for i in index) > R.DENSE_MIN_ROIS == 18432, per_frame


def test_stale_sequence_is_what_it_says():
    big, cut, one = R.stale_sequence()
    assert len(big) == 9 and len(cut) == 8 and len(one) == 9 and np.array_equal(cut, big[:8])
    for batch, n in ((big, 130), (cut, 130), (one, 1)):   # (the ninth frame of the 130-crop batch is empty)
        kinds = [k for f in batch for k in B.ring_kinds(f, np.ascontiguousarray(f[..., 0]))]
        assert len(kinds) == n and (n == 1 or {k[4] for k in kinds} == {0, 1}), (n, len(kinds))


# ---- the rectangle of a clean ring is never a quad ----------------------------------------------------------------------------
def ring_rect_pairs():
    """(sw, sh) of every plane with 8 <= sw, sh <= 600, sw even; 2000 seeded pairs up to 32766; the extremes of both axes"""
    sw, sh = [a.ravel() for a in np.meshgrid(np.arange(8, 601, 2), np.arange(8, 601))]
    rng = np.random.default_rng(20261020)
    rw, rh = rng.integers(4, 16384, 2000) * 2, rng.integers(8, 32767, 2000)
    ew, eh = [8, 8, 32766, 32766], [8, 32766, 8, 32766]
    return np.concatenate([sw, rw, ew]).astype(np.int32), np.concatenate([sh, rh, eh]).astype(np.int32)


def test_ring_rectangle_is_never_a_quad(emul):
    """(1,1) (1,sh-2) (sw-2,sh-2) (sw-2,1) through the oracle's approximation and through the device's own (trace_core.h, as
    follow.hip::approximate_and_emit calls it), at 0.02 of the perimeter: each gives 2 vertices, or 4 that begin with (1, 1), and
    trace_core.h::quad_filter rejects each for every image the plane can be cut from (img_w in {sw, sw+1}, img_h in {sh, sh+1})"""
    sw, sh = ring_rect_pairs()
    n = len(sw)
    assert n > 150000 and sw.min() == sh.min() == 8 and sw.max() == sh.max() == 32766 and not (sw & 1).any()
    dev_m, dev_p, acc = np.zeros(n, np.int32), np.zeros((n, 8), np.int32), np.zeros(n, np.int32)
    emul.emul_ring_rects(n, P(sw), P(sh), P(dev_m), P(dev_p))
    o = H.oracle()
    orc_m, orc_p = np.zeros(n, np.int32), np.zeros((n, 8), np.int32)
    src, dst = np.zeros(8, np.int32), np.zeros(64, np.int32)
    ps, pd = P(src), P(dst)
    for i in range(n):
        a, b = int(sw[i]), int(sh[i])
        src[:] = (1, 1, 1, b - 2, a - 2, b - 2, a - 2, 1)
        orc_m[i] = o.orc_approx_poly(ps, 4, o.orc_arc_length_closed(ps, 4) * 0.02, pd)
        orc_p[i] = dst[:8]
    for what, m, p in (("oracle", orc_m, orc_p), ("device", dev_m, dev_p)):
        assert set(np.unique(m).tolist()) <= {2, 4}, (what, np.unique(m))
        four = m == 4
        assert four.any() and (p[four, :2] == 1).all(), what
        emul.emul_quad_filter_rois(n, P(sw), P(sh), P(m), P(p), P(acc))
        assert not acc.any(), (what, sw[acc != 0][:8], sh[acc != 0][:8], acc[acc != 0][:8])
    assert np.array_equal(orc_m, dev_m) and np.array_equal(orc_p[orc_m == 4], dev_p[dev_m == 4])
    # (the filter is not rejecting everything: the same rectangle begun at its far corner passes where that corner is inside)
    q = np.array([[38, 38, 38, 1, 1, 1, 1, 38]], np.int32)
    one, four = np.array([40], np.int32), np.array([4], np.int32)
    emul.emul_quad_filter_rois(1, P(one), P(one), P(four), P(q), P(acc))
    assert acc[0] == 1 << 3   # img_w = img_h = 41 alone

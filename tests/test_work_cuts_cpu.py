"""CPU tests of the case tables of tests/work_cut_scenes.py: from the oracle's quads and the host build of the batch plan alone,
every class of work cut that tests/test_gpu_work_cuts.py is there for is present in its scenes.  A class that went missing --
a changed scene, a changed plan -- fails here instead of being passed over on the GPU."""
import numpy as np
import pytest

import helpers as H
import work_cut_scenes as S
from test_batch_plan_cpu import lib, plan   # noqa: F401  (lib: the fixture that builds tests/emul/plan_emul.cpp)


def oracle_crops(name):
    W, Hh, frames, want = S.crop_scene(name)
    return W, Hh, want, [S.crop_rois(H.oracle_find_squares(np.ascontiguousarray(f[..., 0])), W, Hh) for f in frames]


@pytest.mark.parametrize("name", sorted(S.CROP_SCENES))
def test_crop_scene_reaches_its_classes(name):
    W, Hh, want, per_frame = oracle_crops(name)
    got = S.crop_classes(per_frame, W, Hh)
    assert want <= got, (name, sorted(want - got))
    assert W <= 560 and Hh <= 560
    assert max(len(p) for p in per_frame) <= 256   # (what a plain context keeps per frame)


def test_crop_scenes_cover_every_class():
    got = set()
    for name in S.CROP_SCENES:
        W, Hh, _, per_frame = oracle_crops(name)
        got |= S.crop_classes(per_frame, W, Hh)
    assert S.CROP_CLASSES <= got, sorted(S.CROP_CLASSES - got)


def test_bars_bracket_the_smallest_crops_the_square_finder_yields():
    """the thinnest bars of the edge scene give no crop, thicker ones do: the shortest and the narrowest crop of the scene are the
    smallest the square finder yields on such a shape, and both lie on the byte-load side of sw = 32"""
    W, Hh, _, per_frame = oracle_crops("edges")
    bars = per_frame[-len(S.BAR_THICKNESS):]
    low = [min([r[4] & ~1 for r in p], default=None) for p in bars]    # shortest crop of each bar frame
    thin = [min([r[3] & ~1 for r in p], default=None) for p in bars]   # narrowest
    assert low[0] is None and thin[0] is None, (low, thin)
    assert any(v is not None for v in low), low
    first = next(k for k, v in enumerate(low) if v is not None)
    assert all(v is not None for v in low[first:]) and all(v is not None for v in thin[first:]), (low, thin)
    assert low[first] == min(v for v in low if v is not None) < 32
    assert thin[first] == min(v for v in thin if v is not None) < 32


def test_chunk_cases_reach_their_classes(lib):   # noqa: F811
    got_all = set()
    for width, height, min_units, formats, want in S.CHUNK_CASES:
        d = plan(lib, width, height, 1, max_batch=9)
        p = d if min_units is None else plan(lib, width, height, 1, max_batch=9, min_units=min_units)
        got = S.chunk_classes(width, height, min_units, d, p)
        assert want <= got, ((width, height, min_units), sorted(want - got), sorted(got))
        got_all |= got
        # 9 frames: the same cut (min_units scaled by the frames, as the GPU test sets it)
        p9 = plan(lib, width, height, 9, max_batch=9) if min_units is None else plan(lib, width, height, 9, max_batch=9, min_units=9 * min_units)
        assert (p9.frame_chunks, p9.frame_chunk_rows, p9.frame_strips) == (p.frame_chunks, p.frame_chunk_rows, p.frame_strips)
        if "last_2" in want:
            assert p.sh - (p.frame_chunks - 1) * p.frame_chunk_rows == 2 and p.frame_chunk_rows == 140
    assert S.CHUNK_CLASSES <= got_all, sorted(S.CHUNK_CLASSES - got_all)
    assert set(S.CHUNK_CASES[0][3]) == {"bgr", "rgb", "bgra", "rgba", "gray"} and "last_2" in S.CHUNK_CASES[0][4]
    # the smallest height with a 2-row last chunk under the default plan
    heights = [h for h in range(16, 1263, 2) if (lambda o: o.sh - (o.frame_chunks - 1) * o.frame_chunk_rows)(plan(lib, 64, h, 1)) == 2]
    assert heights == [1262]


def test_chunk_frames_have_a_marker_across_every_seam(lib):   # noqa: F811
    for width, height, min_units, _, _ in S.CHUNK_CASES:
        p = plan(lib, width, height, 1, max_batch=9) if min_units is None else plan(lib, width, height, 1, max_batch=9, min_units=min_units)
        seams = S.seam_rows(p)
        fr = S.chunk_frames(width, height, seams, 3)
        assert fr.shape == (2, height, width, 3)
        flat = S.textured(width, height, 3 + 1)
        drawn = (fr[1][..., 0] != flat)
        for r in seams:   # the rows on either side of a seam carry marker pixels, dark ones among them
            for row in (r - 1, r):
                assert drawn[row].sum() >= 20 and (fr[1][row, :, 0] == 20).any(), (width, height, min_units, r, row)


def test_plan_scene_is_eight_distinct_frames_and_foreign_poison():
    frames, poison = S.plan_scene()
    assert frames.shape == poison.shape == (8, 240, 320, 3)
    every = [f.tobytes() for f in frames] + [f.tobytes() for f in poison]
    assert len(set(every)) == 16
    # the oracle finds markers in the marker frames; the sawtooth frame has borders of more steps than tier 1's 96 and than the
    # 128 that tier 2 gets in batches of up to 8 frames (and under the mid_steps settings the GPU test makes), fewer than its 1536
    tpls, cam = H.oracle_templates(), H.oracle_camera(320, 240)
    assert all(len(H.oracle_registration(frames[k], tpls, cam)[0]) >= 1 for k in range(6))
    cont, _, _ = H.oracle_contours(H.oracle_binarise(np.ascontiguousarray(frames[6][..., 0])))
    steps = [int(np.abs(np.diff(np.vstack([c, c[:1]]), axis=0)).max(1).sum()) for c in cont]
    assert sum(128 < s <= 1536 for s in steps) >= 3 and max(steps) > 1024, sorted(steps)[-6:]

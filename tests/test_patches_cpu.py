"""The patch core (opencv-ar_amd/csrc/patch_core.h) on the host: byte for byte against the oracle's
cvGetPerspectiveTransform + cvWarpPerspective, exact copies where the map is a translation, and the status rule."""
import numpy as np
import pytest

import frame_kit as FK
import patch_chain as PC
from frame_kit import FMTS

W, Hh = 320, 240
PER_COMBO = 50   # records per (format, patch size): 5 x 8 x 50 = 2000


@pytest.fixture(scope="module")
def L():
    return PC.build_emul()


def test_oracle_parity_on_random_quads(L):
    """Patches whose float32 map equals the oracle's (Jacobi SVD) are the oracle chain's bytes; the others -- last-bit ties of the
    two solvers, at most 5 % (0.98 % of 20 000 when the core was written) -- are the oracle's warp under the core's map."""
    rng = np.random.default_rng(2024)
    total = ties = 0
    for fi, fmt in enumerate(FMTS):
        fr = FK.Frames(1, W, Hh, fmt, row_pad=3, seed=100 + fi)
        planes = PC.planes_of(fr, 0)
        for pw, ph in PC.SIZES:
            quads = PC.random_quads(rng, PER_COMBO, W, Hh)
            recs = FK.records(quads)[None]
            pt, out, status = PC.host_patches(L, fr, recs, [PER_COMBO], pw, ph)
            assert (status == 1).all()
            got = pt.view(out)[0]
            for k in range(PER_COMBO):
                mc, mo = PC.core_map32(L, quads[k], pw, ph), PC.oracle_map32(quads[k], pw, ph)
                same_map = mc.tobytes() == mo.tobytes()
                want = PC.oracle_warp(planes, mo if same_map else mc, pw, ph)
                assert (got[k] == want).all(), (fmt, pw, ph, k, same_map, int((got[k] != want).sum()))
                total += 1
                ties += not same_map
    print("maps that differ from the oracle's: %d of %d" % (ties, total))
    assert total == 2000 and ties <= 0.05 * total, (ties, total)


@pytest.mark.parametrize("fmt", FMTS)
def test_a_square_on_pixel_centres_copies_the_pixels(L, fmt):
    """axis_square(x0, y0, pw, ph) with a pw x ph patch: the map is the exact translation, every fraction is 0"""
    fr = FK.Frames(1, 61, 37, fmt, row_pad=5, seed=7)
    img = fr.view(0)
    for (pw, ph), (x0, y0) in [((16, 16), (3, 4)), ((3, 5), (58, 32)), ((2, 2), (0, 0)), ((61, 37), (0, 0)), ((17, 9), (20, 11))]:
        recs = FK.records([FK.axis_square(x0, y0, pw, ph)])[None]
        for flags in (0, PC.FLIP_ROWS):
            pt, out, status = PC.host_patches(L, fr, recs, [1], pw, ph, flags)
            want = img[y0:y0 + ph, x0:x0 + pw]
            assert status[0, 0] == 1
            assert (pt.view(out)[0, 0] == (want[::-1] if flags else want)).all(), (pw, ph, x0, y0, flags)
    # hanging over the bottom-right corner of the frame: the outside part is 0
    pw, ph, x0, y0 = 16, 12, 61 - 7, 37 - 5
    pt, out, _ = PC.host_patches(L, fr, FK.records([FK.axis_square(x0, y0, pw, ph)])[None], [1], pw, ph)
    want = np.zeros((ph, pw, fr.bpp), np.uint8)
    want[:5, :7] = img[y0:, x0:]
    assert (pt.view(out)[0, 0] == want).all()
    # and over the top-left one
    pt, out, _ = PC.host_patches(L, fr, FK.records([FK.axis_square(-4, -3, pw, ph)])[None], [1], pw, ph, PC.FLIP_ROWS)
    want = np.zeros((ph, pw, fr.bpp), np.uint8)
    want[3:, 4:] = img[:ph - 3, :pw - 4]
    assert (pt.view(out)[0, 0] == want[::-1]).all()


def status_records():
    """eight records and what the status rule makes of them without / with MATCHED_ONLY"""
    good = FK.axis_square(5, 6, 20, 20)
    collinear = [3, 3, 9, 9, 15, 15, 21, 21]
    nan, inf, far = list(good), list(good), list(good)
    nan[3], inf[4], far[6] = np.nan, -np.inf, 2e6
    outside = [-400, -300, -380, -300, -380, -280, -400, -280]
    recs = FK.records([good, collinear, nan, inf, far, good, outside, good], scores=[1, 1, 1, 1, 1, 0, 1, 1])
    return recs, [1, 0, 0, 0, 0, 1, 1, 1], [1, 0, 0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("fmt", ["gray", "bgr", "rgba"])
def test_status_rule_and_untouched_bytes(L, fmt):
    fr = FK.Frames(4, 64, 48, fmt, seed=11)
    base, plain, matched = status_records()
    recs = np.stack([base] * 4)
    counts = [0, 8, 10 ** 6, 5]   # none; all; above the stride, read as it; the first five
    pw, ph = 16, 9
    for flags, rule in ((0, plain), (PC.MATCHED_ONLY, matched), (PC.MATCHED_ONLY | PC.FLIP_ROWS, matched)):
        pt, out, status = PC.host_patches(L, fr, recs, counts, pw, ph, flags)
        want = np.array([[0] * 8, rule, rule, rule[:5] + [0, 0, 0]])
        assert (status == want).all(), (flags, status.tolist())
        v = pt.view(out)
        assert (v[want == 0] == FK.GUARD).all()                      # a slot that is not written keeps every byte
        assert (out[:pt.lead] == FK.GUARD).all() and (out[out.size - FK.LEAD:] == FK.GUARD).all()
        assert (v[1:3, 6] == 0).all()                                # wholly outside the frame: zeros, status 1
        assert (v[1, 0] != FK.GUARD).any() and (v[1, 0] == v[1, 7]).all()
        if not flags:
            assert (v[1, 5] == v[1, 0]).all()                        # score 0 is extracted unless MATCHED_ONLY
    # a stride below the count: only the first slots exist
    pt, out, status = PC.host_patches(L, fr, recs, [8] * 4, pw, ph, 0, per_frame=3)
    assert status.shape == (4, 3) and (status == [1, 0, 0]).all()
    assert (pt.view(out)[:, 1:] == FK.GUARD).all()

"""The overlay core (opencv-ar_amd/csrc/overlay_core.h, host build tests/emul/overlay_emul.cpp) against things known
independently: exact copies and quarter turns, the weight formula at magnification two, the blend formula in every format, the
composition order, the records that draw nothing, and a float64 restatement of the homography on random perspective quads.
Every frame carries guard bytes in its row padding and around the buffer; they must survive.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import overlay_chain as OC
from helpers import P


@pytest.fixture(scope="module")
def L():
    return OC.build_emul()


def render(L, fr, squares, overlays, tids=None, scores=None, count=None):
    recs = FK.records(squares, tids, scores)[None]
    out, drawn = OC.host_render(L, fr, recs, [len(recs[0]) if count is None else count], overlays)
    guards = ~fr.pixel_mask()
    assert (out[guards] == FK.GUARD).all(), "guard bytes changed"
    return fr.view(0, out), drawn[0]


@pytest.mark.parametrize("ow,oh", [(2, 2), (3, 5), (17, 9)])
def test_opaque_overlay_on_its_own_rectangle_is_an_exact_copy(L, ow, oh):
    rng = np.random.default_rng(ow * 100 + oh)
    ov = OC.random_overlay(rng, ow, oh, alpha=255)
    fr = FK.Frames(1, 40, 30, "rgb", row_pad=5)
    x0, y0 = 7, 11
    got, drawn = render(L, fr, [FK.axis_square(x0, y0, ow, oh)], {0: ov})
    assert drawn == 1
    want = fr.view(0).copy()
    want[y0:y0 + oh, x0:x0 + ow] = ov[..., :3]
    assert (got == want).all()


def test_cyclic_shifts_of_the_corners_give_the_four_quarter_turns(L):
    rng = np.random.default_rng(5)
    n = 6
    ov = OC.random_overlay(rng, n, n, alpha=255)
    sq = np.array(FK.axis_square(10, 8, n, n), np.float32).reshape(4, 2)
    for s in range(4):
        fr = FK.Frames(1, 32, 24, "rgb")
        got, _ = render(L, fr, [np.roll(sq, -s, axis=0)], {0: ov})   # new corner i = old corner i + s
        want = fr.view(0).copy()
        want[8:8 + n, 10:10 + n] = np.rot90(ov[..., :3], -s)
        assert (got == want).all(), s


def test_magnification_by_two_follows_the_weight_formula(L):
    rng = np.random.default_rng(6)
    ow, oh = 5, 4
    ov = OC.random_overlay(rng, ow, oh, alpha=255)
    W, Hh = 2 * (ow - 1) + 1, 2 * (oh - 1) + 1
    fr = FK.Frames(1, 20, 16, "rgba", row_pad=3)
    got, _ = render(L, fr, [FK.axis_square(3, 2, W, Hh)], {0: ov})
    t = ov.astype(np.int64)
    want = np.zeros((Hh, W, 4), np.int64)
    want[0::2, 0::2] = t
    want[0::2, 1::2] = (t[:, :-1] * 512 + t[:, 1:] * 512 + 512) >> 10
    want[1::2, 0::2] = (t[:-1] * 512 + t[1:] * 512 + 512) >> 10
    want[1::2, 1::2] = ((t[:-1, :-1] + t[:-1, 1:] + t[1:, :-1] + t[1:, 1:]) * 256 + 512) >> 10
    assert (want[..., 3] == 255).all()
    exp = fr.view(0).copy()
    exp[2:2 + Hh, 3:3 + W, :3] = want[..., :3]
    assert (got == exp).all()   # (byte 3 of the RGBA frame included: untouched)


@pytest.mark.parametrize("fmt", ["bgr", "rgb", "bgra", "rgba", "gray"])
def test_alpha_follows_the_blend_formula_in_every_format(L, fmt):
    rng = np.random.default_rng(7)
    ow = oh = 8
    ov = OC.random_overlay(rng, ow, oh, alpha=255)
    ov[:, 0:3, 3] = 0
    ov[:, 3:6, 3] = 128
    fr = FK.Frames(1, 24, 20, fmt, row_pad=5, seed=3)
    x0, y0 = 5, 6
    got, _ = render(L, fr, [FK.axis_square(x0, y0, ow, oh)], {0: ov})
    exp = fr.view(0).copy()
    region = exp[y0:y0 + oh, x0:x0 + ow]
    nc = 1 if fmt == "gray" else 3
    col = OC.colour_in_format(ov, fmt)
    if fmt == "gray":   # the library's grey, by the oracle's own conversion
        bgr = np.ascontiguousarray(ov[..., [2, 1, 0]])
        g = np.zeros((oh, ow), np.uint8)
        H.oracle().orc_bgr2gray(P(bgr), ow, oh, ow * 3, P(g), ow)
        assert (col[..., 0] == g).all()
    a = ov[..., 3].astype(np.int64)[..., None]
    blended = OC.blend(col, a, region[..., :nc])
    region[..., :nc] = np.where(a > 0, blended, region[..., :nc])
    assert (got == exp).all()
    assert (got[y0:y0 + oh, x0:x0 + 3] == fr.view(0)[y0:y0 + oh, x0:x0 + 3]).all()   # alpha 0 wrote nothing
    if fmt in ("bgra", "rgba"):
        assert (got[..., 3] == fr.view(0)[..., 3]).all()


def test_overlapping_records_compose_in_output_order(L):
    ca, cb = np.array([200, 30, 90, 128], np.uint8), np.array([10, 220, 160, 128], np.uint8)
    ovs = {0: np.broadcast_to(ca, (2, 2, 4)).copy(), 1: np.broadcast_to(cb, (2, 2, 4)).copy()}
    fr = FK.Frames(1, 40, 30, "rgb", seed=8)
    sa, sb = FK.axis_square(4, 4, 20, 16), FK.axis_square(14, 10, 20, 16)
    got, drawn = render(L, fr, [sa, sb], ovs, tids=[0, 1])
    assert drawn == 2
    exp = fr.view(0).astype(np.int64)
    exp[4:20, 4:24] = OC.blend(ca[:3], 128, exp[4:20, 4:24])
    exp[10:26, 14:34] = OC.blend(cb[:3], 128, exp[10:26, 14:34])
    assert (got == exp).all()
    rev, _ = render(L, fr, [sb, sa], ovs, tids=[1, 0])
    assert (rev != got).any() and (rev[4:10] == got[4:10]).all()


NOTHING = {
    "outside": ([-60, -50, -30, -50, -30, -20, -60, -20], 0, 1.0),
    "outside right": ([100, 5, 130, 5, 130, 25, 100, 25], 0, 1.0),
    "collinear": ([2, 2, 10, 10, 20, 20, 30, 30], 0, 1.0),
    "three in a line": ([2, 2, 10, 2, 20, 2, 10, 20], 0, 1.0),
    "equal adjacent": ([5, 5, 5, 5, 25, 25, 5, 25], 0, 1.0),
    "equal opposite": ([5, 5, 25, 6, 5, 5, 6, 25], 0, 1.0),
    "nan": ([5, 5, np.nan, 5, 25, 25, 5, 25], 0, 1.0),
    "inf": ([5, 5, 25, 5, np.inf, 25, 5, 25], 0, 1.0),
    "score 0": ([5, 5, 25, 5, 25, 25, 5, 25], 0, 0.0),
    "score nan": ([5, 5, 25, 5, 25, 25, 5, 25], 0, np.nan),
    "no overlay": ([5, 5, 25, 5, 25, 25, 5, 25], 3, 1.0),
}


@pytest.mark.parametrize("case", sorted(NOTHING))
def test_records_that_draw_nothing(L, case):
    sq, tid, score = NOTHING[case]
    ov = OC.random_overlay(np.random.default_rng(9), 4, 4, alpha=255)
    fr = FK.Frames(1, 40, 30, "bgr", row_pad=2)
    got, drawn = render(L, fr, [sq], {0: ov}, tids=[tid], scores=[score])
    assert drawn == 0 and (got == fr.view(0)).all()


def test_count_zero_draws_nothing_and_the_default_overlay_serves_the_rest(L):
    ov = OC.random_overlay(np.random.default_rng(10), 4, 4, alpha=255)
    fr = FK.Frames(1, 40, 30, "bgr")
    sq = FK.axis_square(5, 5, 4, 4)
    got, drawn = render(L, fr, [sq], {0: ov}, count=0)
    assert drawn == 0 and (got == fr.view(0)).all()
    got, drawn = render(L, fr, [sq], {-1: ov}, tids=[3])   # template 3 has none of its own
    assert drawn == 1 and (got[5:9, 5:9] == ov[..., [2, 1, 0]]).all()
    own = OC.random_overlay(np.random.default_rng(11), 4, 4, alpha=255)
    got, _ = render(L, fr, [sq], {-1: ov, 3: own}, tids=[3])   # its own overlay wins
    assert (got[5:9, 5:9] == own[..., [2, 1, 0]]).all()


@pytest.mark.parametrize("x0,y0", [(-6, 4), (30, 4), (10, -5), (10, 22), (-6, -5), (30, 22)])
def test_a_square_cut_by_the_frame_draws_only_inside(L, x0, y0):
    ow, oh = 16, 12
    ov = OC.random_overlay(np.random.default_rng(12), ow, oh, alpha=255)
    fr = FK.Frames(1, 40, 30, "rgb", row_pad=5)
    got, drawn = render(L, fr, [FK.axis_square(x0, y0, ow, oh)], {0: ov})
    assert drawn == 1
    exp = fr.view(0).copy()
    xa, xb, ya, yb = max(x0, 0), min(x0 + ow, 40), max(y0, 0), min(y0 + oh, 30)
    exp[ya:yb, xa:xb] = ov[ya - y0:yb - y0, xa - x0:xb - x0, :3]
    assert (got == exp).all()


def homography(src, dst):
    """float64 H with H (src, 1) ~ (dst, 1) for four point pairs"""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y])
        b += [u, v]
    h = np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))
    return np.append(h, 1.0).reshape(3, 3)


def random_convex_quad(rng, width, height):
    while True:
        s = rng.uniform(20, 200)
        c = np.array([rng.uniform(0.2, 0.8) * width, rng.uniform(0.2, 0.8) * height])
        ang = rng.uniform(0, 2 * np.pi) + np.arange(4) * np.pi / 2 + np.pi / 4
        q = c + s / np.sqrt(2) * np.stack([np.cos(ang), np.sin(ang)], 1) + rng.uniform(-0.2, 0.2, (4, 2)) * s
        e = np.roll(q, -1, axis=0) - q
        z = [e[i, 0] * e[(i + 1) % 4, 1] - e[i, 1] * e[(i + 1) % 4, 0] for i in range(4)]
        sides = [np.hypot(*(q[(i + 1) % 4] - q[i])) for i in range(4)]
        if (min(z) > 0 or max(z) < 0) and min(sides) >= 20 and max(sides) <= 200:
            return q.astype(np.float32)


def test_perspective_quads_against_a_float64_homography(L):
    """Twenty random convex quads of 20 .. 200 px sides on a 320 x 240 frame, an opaque overlay of linear ramps (at most one level
    per texel).  Against the exact homography in float64 with unquantised bilinear sampling: covered pixels within 2 levels
    (1/64-texel coordinate quantisation of ramps of <= 1 level per texel: 1/64 level each way, two roundings: 1/2 + 1/2, the
    float32 matrix: << 1), coverage equal except where (u, v) lies within 1/16 texel of the rectangle's border."""
    rng = np.random.default_rng(20)
    ow, oh = 96, 64
    i, j = np.meshgrid(np.arange(ow), np.arange(oh))
    ov = np.stack([i, j * 2 // 3 + 20, np.full_like(i, 255), np.full_like(i, 255)], -1).astype(np.uint8)   # B = 255 marks coverage
    W, Hh = 320, 240
    ys, xs = np.mgrid[0:Hh, 0:W]
    for n in range(20):
        q = random_convex_quad(rng, W, Hh)
        fr = FK.Frames(1, W, Hh, "rgb", fill=0)
        got, drawn = render(L, fr, [q.reshape(8)], {0: ov})
        assert drawn == 1
        Hm = homography(q.astype(np.float64), [(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)])
        w = Hm[2, 0] * xs + Hm[2, 1] * ys + Hm[2, 2]
        u = (Hm[0, 0] * xs + Hm[0, 1] * ys + Hm[0, 2]) / w
        v = (Hm[1, 0] * xs + Hm[1, 1] * ys + Hm[1, 2]) / w
        ref_cov = (u >= 0) & (u <= ow - 1) & (v >= 0) & (v <= oh - 1)
        cov = got[..., 2] == 255
        border = np.minimum(np.minimum(np.abs(u), np.abs(u - (ow - 1))), np.minimum(np.abs(v), np.abs(v - (oh - 1))))
        near = (border <= 1 / 16) & (u >= -1 / 16) & (u <= ow - 1 + 1 / 16) & (v >= -1 / 16) & (v <= oh - 1 + 1 / 16)
        assert ((cov != ref_cov) <= near).all(), n
        both = cov & ref_cov
        assert both.sum() > 200
        uu, vv = np.clip(u[both], 0, ow - 1), np.clip(v[both], 0, oh - 1)
        ix, iy = np.minimum(uu.astype(int), ow - 2), np.minimum(vv.astype(int), oh - 2)
        fx, fy = (uu - ix)[:, None], (vv - iy)[:, None]
        t = ov[..., :2].astype(np.float64)
        ref = (t[iy, ix] * (1 - fx) + t[iy, ix + 1] * fx) * (1 - fy) + (t[iy + 1, ix] * (1 - fx) + t[iy + 1, ix + 1] * fx) * fy
        diff = np.abs(got[both][:, :2].astype(np.float64) - ref)
        print("quad %d: %d px, max difference %.3f levels, %d coverage differences" % (n, both.sum(), diff.max(), (cov != ref_cov).sum()))
        assert diff.max() <= 2.0, n

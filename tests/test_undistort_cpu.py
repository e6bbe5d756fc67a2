"""The undistortion core (opencv-ar_amd/csrc/undistort_core.h) on the host (tests/undistort_chain.py builds it): what the two
maps compute, without a device -- a lens of zeros copies, the border is a constant 0, the record map inverts the frame map,
every channel is remapped alike, and the oracle finds on an undistorted view of a distorting camera what it finds on the pinhole
view.  tests/test_gpu_undistort.py holds the kernels to this build byte for byte."""
import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import persp_synth as PS
import undistort_chain as UC

SIZES = [(33, 17), (320, 240)]


@pytest.fixture(scope="module")
def L():
    return UC.build_emul()


def odd_records(rng, n, W, Hh):
    """n records with random squares around the frame, every field filled, one NaN and one 1e30 coordinate among them"""
    r = FK.records(rng.uniform(-20, max(W, Hh) + 20, (n, 8)), template_ids=rng.integers(0, 9, n), scores=rng.integers(0, 2, n))
    r["glMatrix"] = rng.normal(size=(n, 16))
    r["aspectRatio"] = rng.uniform(0.5, 2, n)
    if n >= 3:
        r["square"][1, 3] = np.nan
        r["square"][2, 0] = 1e30
    return r


@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("size", SIZES)
def test_a_lens_of_zeros_copies_frames_and_records(L, fmt, size):
    W, Hh = size
    cam = UC.camera(W, Hh, "ZERO")
    src = FK.Frames(2, W, Hh, fmt, row_pad=3, frame_gap=8, seed=W)
    dst = UC.dst_frames(2, W, Hh, fmt, row_pad=1, lead=FK.LEAD + 1)
    out = UC.host_undistort(L, src, cam, dst)
    for f in range(2):
        assert (dst.view(f, out) == src.view(f)).all()
    assert (out[~dst.pixel_mask()] == FK.GUARD).all()
    recs = odd_records(np.random.default_rng(W), 6, W, Hh).reshape(2, 3)
    assert UC.host_records(L, cam, recs, [3, 2]).tobytes() == recs.tobytes()


def fixed_point(L, cam, W, Hh):
    """(X, Y) of every destination pixel as the core defines them, [H, W] int64 each: restated from the frame map's (us, vs)"""
    v, u = np.mgrid[0:Hh, 0:W]
    s = UC.frame_map(L, cam, np.stack([u.ravel(), v.ravel()], 1))
    q = np.rint(np.clip(32 * s, -2147483648.0, 2147483647.0)).astype(np.int64)
    return q[:, 0].reshape(Hh, W), q[:, 1].reshape(Hh, W)


def white_frame_expected(X, Y, W, Hh):
    """the sampler on an all-255 frame: the 15-bit weights of the taps inside the frame -> (bytes, all four taps outside)"""
    ix, iy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    w = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    exact = (fx | fy) == 0
    w[0], w[3] = np.where(exact, 32767, w[0]), np.where(exact, 1, w[3])
    x_in = [(ix >= 0) & (ix < W), (ix + 1 >= 0) & (ix + 1 < W)]
    y_in = [(iy >= 0) & (iy < Hh), (iy + 1 >= 0) & (iy + 1 < Hh)]
    inside = [x_in[0] & y_in[0], x_in[1] & y_in[0], x_in[0] & y_in[1], x_in[1] & y_in[1]]
    total = sum(np.where(m, wk, 0) for m, wk in zip(inside, w))
    return ((255 * total + 16384) >> 15).astype(np.uint8), ~(inside[0] | inside[1] | inside[2] | inside[3])


def test_the_border_is_a_constant_zero(L):
    W, Hh = 320, 240
    white = np.full((Hh, W), 255, np.uint8)
    cam = UC.camera(W, Hh, "PINCUSHION")
    out = UC.host_undistort_image(L, white, cam)
    want, all_out = white_frame_expected(*fixed_point(L, cam, W, Hh), W, Hh)
    assert (out == want).all()
    assert set(np.unique(out[all_out])) == {0} and (out == 255).any()
    # zero nowhere else, but for taps of vanishing weight on the very rim (255 w + 16384 < 32768)
    rim = (out == 0) & ~all_out
    print("PINCUSHION 320x240: %.2f %% of the pixels have all taps outside, %d more are 0 on the rim" % (100 * all_out.mean(), rim.sum()))
    assert 0.05 < all_out.mean() < 0.2 and rim.sum() < 0.01 * all_out.sum()
    assert not white_frame_expected(*fixed_point(L, UC.camera(W, Hh, "BARREL"), W, Hh), W, Hh)[1].any()   # (BARREL: nothing outside)
    # WILD: the coordinates leave the int range, the clamp keeps the casts defined, and every byte is 0 -- but for the handful of
    # pixels within 2 px of the principal point (160, 120), which the lens model itself leaves inside the frame (r2 of a few 1e-5:
    # even k1 = 1e6 moves them by pixels only); those are held to the restated sampler
    wild = UC.camera(W, Hh, "WILD")
    X, Y = fixed_point(L, wild, W, Hh)
    assert (np.abs(X) >= 2147483647).any() and (np.abs(Y) >= 2147483647).any()
    want, all_out = white_frame_expected(X, Y, W, Hh)
    v, u = np.mgrid[0:Hh, 0:W]
    near = (u - 160) ** 2 + (v - 120) ** 2 <= 4
    assert all_out[~near].all() and near.sum() == 13
    out = UC.host_undistort_image(L, white, wild)
    assert (out == want).all() and not out[~near].any()
    out4 = UC.host_undistort_image(L, np.full((Hh, W, 4), 255, np.uint8), wild)
    assert (out4 == want[..., None]).all()


@pytest.mark.parametrize("lens", ["BARREL", "PINCUSHION"])
def test_the_record_map_inverts_the_frame_map(L, lens):
    """every integer pixel through the record map (rounded to float32 as records are), then through the frame map, comes back
    within one step of the frame map's fixed point, 1/32 px"""
    W, Hh = 320, 240
    cam = UC.camera(W, Hh, lens)
    v, u = np.mgrid[0:Hh, 0:W]
    p = np.stack([u.ravel(), v.ravel()], 1).astype(np.float64)
    back = UC.frame_map(L, cam, UC.record_map(L, cam, p).astype(np.float32).astype(np.float64))
    err = np.abs(back - p).max()
    print("%s 320x240: record map, then frame map: at most %.3g px from the pixel" % (lens, err))
    assert err < 1.0 / 32


def test_every_channel_is_remapped_alike(L):
    W, Hh = 61, 37
    img = np.random.default_rng(4).integers(0, 256, (Hh, W, 4), dtype=np.uint8)
    for lens in ("BARREL", "PINCUSHION", "OFF_CENTRE"):
        cam = UC.camera(W, Hh, lens)
        out = UC.host_undistort_image(L, img, cam)
        for c in range(4):
            assert (out[..., c] == UC.host_undistort_image(L, np.ascontiguousarray(img[..., c]), cam)).all(), (lens, c)
        assert (out != img).any()


# ---- meaning: the oracle on an undistorted view ----------------------------------------------------------------------------------

MEANING_SCENES = ("ladder-160-0", "ladder-160-2")


@pytest.fixture(scope="module")
def pinhole_scenes():
    tpls = H.oracle_templates(PS.NAMES)
    scenes = [s for s in PS.ladder(lens=False, sizes=(160,)) if s.name in MEANING_SCENES]
    assert [s.name for s in scenes] == list(MEANING_SCENES)
    return tpls, [(s, H.oracle_registration(s.frame, tpls, s.cam)[0]) for s in scenes]


@pytest.mark.parametrize("lens", ["BARREL", "PINCUSHION"])
def test_the_oracle_finds_on_the_undistorted_view_what_it_finds_on_the_pinhole_view(L, pinhole_scenes, lens):
    """a 960 x 540 pinhole frame, distorted in numpy (a truly distorted image), undistorted by the host build: the oracle with the
    pinhole camera gives the same number of records, the same templates and scores, corners within 2 px (1 px with a float sampler;
    the second is the margin for the fixed-point sampler's last grey level)"""
    tpls, scenes = pinhole_scenes
    for s, ref in scenes:
        cam = UC.camera(s.width, s.height, lens)
        D = UC.distort_image(s.frame, cam)
        assert np.abs(D.astype(int) - s.frame).max() > 100   # (the markers moved)
        got = H.oracle_registration(UC.host_undistort_image(L, D, cam), tpls, s.cam)[0]
        assert len(ref) >= 2 and len(got) == len(ref), (s.name, lens, len(got), len(ref))
        by_tpl = {m.templateId: m for m in got}
        worst = 0.0
        for r in ref:
            m = by_tpl.get(r.templateId)
            assert m is not None and m.score == r.score, (s.name, lens, r.templateId)
            worst = max(worst, float(np.abs(np.array(m.square) - np.array(r.square)).max()))
        print("%s %s: corners within %.3f px of the pinhole frame's" % (s.name, lens, worst))
        assert worst <= 2.0, (s.name, lens, worst)

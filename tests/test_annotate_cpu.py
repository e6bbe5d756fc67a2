"""The annotation core on the host (opencv-ar_amd/csrc/annotate_core.h through tests/emul/annotate_emul.cpp): stroke coverage
against a numpy float64 restatement, compositing, which records draw, the projected pose primitives, the label, the style's
refusals, the stand-alone sanitizer program and the ABI surface.  The stroke rule is the library's own: nothing here compares
with OpenCV's line rasteriser."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import annotate_chain as AC
import frame_kit as FK
import helpers as H
import overlay_chain as OC
import persp_synth as PS
from hostbuild import run_sanitized


@pytest.fixture(scope="module")
def L():
    return AC.build_emul()


def one_frame(L, W, Hh, fmt, recs, st, cam=None, fill=0, row_pad=0, count=None):
    fr = FK.Frames(1, W, Hh, fmt, row_pad=row_pad, fill=fill)
    recs = np.asarray(recs).reshape(1, -1)
    out, drawn = AC.host_annotate(L, fr, recs, [recs.shape[1] if count is None else count], st, cam)
    return fr, out, drawn[0]


def segment_record(a, b):
    """a record whose outline is the stroke of the one segment a -- b: corners a, b, b, a (the edges b -- b and a -- a are its caps)"""
    return FK.records([[a[0], a[1], b[0], b[1], b[0], b[1], a[0], a[1]]])


# ---- coverage -----------------------------------------------------------------------------------------------------------------

W0, H0 = 64, 48
SEGMENTS = {
    "horizontal": ((5.0, 20.0), (50.37, 20.0)),
    "horizontal off the rows": ((5.3, 20.3), (50.0, 20.3)),   # (at .45 a 1-px stroke would lie wholly in the free band)
    "vertical": ((30.2, 4.0), (30.2, 41.6)),
    "diagonal": ((8.0, 6.0), (40.0, 38.0)),
    "anti-diagonal": ((45.3, 5.1), (12.3, 38.1)),
    "shallow": ((3.37, 11.81), (59.12, 17.43)),
    "steep": ((22.9, 44.2), (27.15, 2.7)),
    "zero length": ((21.3, 17.1), (21.3, 17.1)),
    "zero length off centre": ((40.2, 30.25), (40.2, 30.25)),
    "out to the left": ((20.0, 24.3), (-17.5, 15.0)),
    "out to the right": ((40.0, 10.0), (91.3, 22.7)),
    "out above": ((31.7, 12.0), (36.2, -25.0)),
    "out below": ((12.0, 30.5), (19.9, 77.0)),
    "through the frame": ((-20.0, -9.0), (90.0, 60.0)),
    "along the top edge": ((-5.0, 0.0), (70.0, 0.2)),
    "along the right edge": ((63.0, -4.0), (63.2, 55.0)),
}


@pytest.mark.parametrize("thickness", [1, 2, 3, 16])
@pytest.mark.parametrize("name", list(SEGMENTS))
def test_a_stroke_is_the_pixels_within_half_the_thickness_of_its_segment(L, name, thickness):
    a, b = SEGMENTS[name]
    st = AC.style(L, AC.OUTLINE, thickness=thickness, outline=(255, 255, 255, 255))
    fr, out, drawn = one_frame(L, W0, H0, "gray", segment_record(a, b), st)
    mask = fr.view(0, out)[..., 0] == 255
    assert set(np.unique(out[fr.pixel_mask()])) <= {0, 255}
    a32, b32 = np.float32(a).astype(np.float64), np.float32(b).astype(np.float64)
    d = AC.np_distance(W0, H0, a32, b32)
    must, never = d <= thickness / 2 - 0.1, d >= thickness / 2 + 0.1
    band = ~must & ~never
    print("%s, thickness %d: %d drawn, %d must, %d in the free band" % (name, thickness, mask.sum(), must.sum(), band.sum()))
    assert mask[must].all(), "missing %d" % (~mask[must]).sum()
    assert not mask[never].any(), "extra %d" % mask[never].sum()
    assert drawn == 1 and band.sum() < mask.sum(), (band.sum(), mask.sum())   # the band cannot swallow a wrong stroke


def test_the_corner_dot_is_a_disc_of_diameter_two_thickness_plus_one(L):
    for t, c in [(1, (20.0, 15.0)), (3, (20.3, 15.6)), (16, (33.0, 24.0))]:
        st = AC.style(L, AC.CORNER0, thickness=t, corner0=(255, 255, 255, 255))
        fr, out, _ = one_frame(L, W0, H0, "gray", FK.records([[c[0], c[1], 50, 10, 50, 40, 10, 40]]), st)
        mask = fr.view(0, out)[..., 0] == 255
        d = AC.np_distance(W0, H0, np.float32(c).astype(np.float64), np.float32(c).astype(np.float64))
        r = (2 * t + 1) / 2
        assert mask[d <= r - 0.1].all() and not mask[d >= r + 0.1].any() and mask.sum() > 0


def test_end_points_round_to_sixteenths_and_clamp(L):
    st = AC.style(L, AC.OUTLINE | AC.CORNER0, thickness=2)
    big = 3.0e7
    ok, rec, box = AC.host_setup(L, FK.records([[10.03, 7.97, big, 5, -big, big, 3.0e38, -3.0e38]])[0], st, 640, 480)
    assert ok
    lim = 16 * AC.MAX_COORD
    assert rec["seg"][0]["a"].tolist() == [160, 128] and rec["seg"][0]["b"].tolist() == [lim, 80]
    assert rec["seg"][1]["b"].tolist() == [-lim, lim] and rec["seg"][2]["b"].tolist() == [lim, -lim]
    assert rec["seg"][AC.SEG_DOT]["a"].tolist() == rec["seg"][AC.SEG_DOT]["b"].tolist() == [160, 128]
    assert rec["seg"][0]["r"] == 16 and rec["seg"][AC.SEG_DOT]["r"] == 8 * 5
    # boxes: grown by the radius, clipped to the frame; the record's box is their union
    assert rec["seg"][0]["box"].tolist() == [9, 4, 639, 9] and box.tolist() == [0, 0, 639, 479]


# ---- compositing --------------------------------------------------------------------------------------------------------------

def test_joints_and_crossings_of_half_transparent_strokes_blend_once(L):
    W, Hh, fill = 96, 80, 90
    cam = PS.camera(W, Hh)
    R, t = PS.pose(cam, 48, 40, 40, 30, 20, 70)
    rec = AC.posed_record(cam, R, t)
    colour = (250, 120, 10, 128)
    st = AC.style(L, AC.OUTLINE | AC.AXES, thickness=3, outline=colour, axis_length=1.6)
    for fmt in ("bgr", "gray"):
        fr, out, drawn = one_frame(L, W, Hh, fmt, [rec], st, cam, fill=fill)
        assert drawn == 1
        img = fr.view(0, out).astype(np.int64)
        changed = (img != fill).any(axis=2)
        once = {tuple(OC.blend(OC.colour_in_format(c, fmt), 128, fill).tolist())
                for c in (colour, (255, 0, 0, 128), (0, 255, 0, 128), (0, 0, 255, 128))}
        seen = {tuple(v) for v in img[changed].tolist()}
        assert seen == once, (fmt, seen - once)   # four colours, each blended exactly once: no joint or crossing darkened twice
    # and an axis does cross an edge: some axis-coloured pixel lies within the outline's stroke
    ok, srec, _ = AC.host_setup(L, rec, st, W, Hh, cam)
    axis_px = (fr.view(0, out)[..., 0] != OC.blend(OC.colour_in_format(colour, "gray"), 128, fill)[0]) & changed
    edge_d = np.min([AC.np_distance(W, Hh, srec["seg"][k]["a"] / 16.0, srec["seg"][k]["b"] / 16.0) for k in range(4)], axis=0)
    assert (axis_px & (edge_d <= 1.3)).any()


def test_later_records_are_drawn_over_earlier_ones(L):
    a = FK.records([FK.axis_square(10, 10, 30, 30), FK.axis_square(25, 10, 30, 30)], [3, 4])
    st = AC.style(L, AC.OUTLINE | AC.COLOR_BY_TEMPLATE, thickness=3)
    pal = [L.annotate_palette_emul(t) for t in (3, 4)]
    assert pal[0] != pal[1]
    fr, out, _ = one_frame(L, 70, 50, "rgb", a, st)
    fr2, out2, _ = one_frame(L, 70, 50, "rgb", a[::-1].copy(), st)
    px = lambda o, x, y: fr.view(0, o)[y, x].tolist()   # noqa: E731
    rgb = lambda w: [w & 255, (w >> 8) & 255, (w >> 16) & 255]   # noqa: E731
    # (25, 10) .. (39, 10) lies on the top edges of both
    assert px(out, 32, 10) == rgb(pal[1]) and px(out2, 32, 10) == rgb(pal[0])
    assert px(out, 12, 10) == rgb(pal[0]) and px(out, 50, 10) == rgb(pal[1])
    # half-transparent: the second is blended over the first
    st.outline[3] = 100
    fr3, out3, _ = one_frame(L, 70, 50, "rgb", a, st, fill=50)
    first = OC.blend(rgb(pal[0]), 100, 50)
    assert px(out3, 32, 10) == OC.blend(rgb(pal[1]), 100, first).tolist()


@pytest.mark.parametrize("fmt", FK.FMTS)
def test_bytes_that_are_never_written(L, fmt):
    W, Hh = 70, 37
    recs = FK.records([FK.axis_square(-4, -3, 40, 30), [60.5, 5, 75, 20, 66, 41, 50, 30]], [12, 345])
    st = AC.style(L, AC.OUTLINE | AC.CORNER0 | AC.LABEL, thickness=2, outline=(10, 200, 90, 255), label=(1, 2, 3, 77))
    fr = FK.Frames(1, W, Hh, fmt, row_pad=5, seed=9)
    out, drawn = AC.host_annotate(L, fr, recs[None], [2], st)
    assert drawn == [2] and (out != fr.buf).any()
    assert (out[~fr.pixel_mask()] == FK.GUARD).all()            # row padding and the bytes around the frame
    if fr.bpp == 4:
        assert (fr.view(0, out)[..., 3] == fr.view(0)[..., 3]).all()   # byte 3
    # alpha 0 touches nothing
    st0 = AC.style(L, AC.OUTLINE | AC.CORNER0 | AC.LABEL, outline=(10, 200, 90, 0), corner0=(255, 0, 0, 0), label=(1, 2, 3, 0))
    out0, drawn0 = AC.host_annotate(L, fr, recs[None], [2], st0)
    assert drawn0 == [2] and (out0 == fr.buf).all()


def test_byte_order_and_grey(L):
    colour = (201, 102, 53, 255)
    st = AC.style(L, AC.OUTLINE, thickness=1, outline=colour)
    rec = FK.records([FK.axis_square(4, 4, 20, 10)])
    got = {}
    for fmt in FK.FMTS:
        fr, out, _ = one_frame(L, 32, 20, fmt, rec, st, fill=7)
        got[fmt] = fr.view(0, out)[4, 10].tolist()
    assert got["rgb"] == [201, 102, 53] and got["bgr"] == [53, 102, 201]
    assert got["rgba"] == [201, 102, 53, 7] and got["bgra"] == [53, 102, 201, 7]
    assert got["gray"] == [int(OC.grey_of(53, 102, 201))]
    # half-transparent: the grey of the colour is blended, not the colour's channels
    st.outline[3] = 99
    fr, out, _ = one_frame(L, 32, 20, "gray", rec, st, fill=7)
    assert fr.view(0, out)[4, 10, 0] == OC.blend(OC.grey_of(53, 102, 201), 99, 7)


def test_a_last_primitive_with_alpha_zero_leaves_the_pixel_alone(L):
    """the pixel takes the colour of the LAST primitive that covers it -- also when that colour is transparent"""
    rec = FK.records([FK.axis_square(10, 10, 20, 20)], [8])
    st = AC.style(L, AC.OUTLINE | AC.CORNER0, thickness=3, outline=(255, 255, 255, 255), corner0=(9, 9, 9, 0))
    fr, out, _ = one_frame(L, 48, 40, "gray", rec, st)
    img = fr.view(0, out)[..., 0]
    assert img[10, 10] == 0 and img[10, 20] == 255 and img[12, 12] == 0   # the dot (radius 3.5) cut a hole into the joint


# ---- which records draw -----------------------------------------------------------------------------------------------------------

def test_counts_and_strides(L):
    sq = [FK.axis_square(4 + 12 * k, 5, 9, 9) for k in range(4)]
    recs = FK.records(sq)
    st = AC.style(L, AC.OUTLINE)
    for count, want in [(0, 0), (1, 1), (3, 3), (4, 4), (5, 4), (10 ** 6, 4), (-1, 0)]:
        _, _, drawn = one_frame(L, 64, 24, "gray", recs, st, count=count)
        assert drawn == want, count


def test_records_that_are_not_finite_or_not_matched(L):
    W, Hh = 64, 48
    base = FK.axis_square(10, 10, 20, 20)
    st = AC.style(L, AC.OUTLINE | AC.CORNER0 | AC.LABEL)
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(8):
            sq = np.array(base, np.float32)
            sq[slot] = bad
            _, out, drawn = one_frame(L, W, Hh, "gray", FK.records([sq]), st, fill=3)
            assert drawn == 0 and (out[FK.LEAD:-FK.LEAD] == 3).all(), (bad, slot)
    un = AC.style(L, AC.OUTLINE | AC.CORNER0 | AC.LABEL | AC.UNMATCHED, unmatched=(77, 77, 77, 255), corner0=(200, 200, 200, 255),
                  outline=(255, 255, 255, 255), label=(150, 150, 150, 255))
    for score, with_flag, without in [(1.0, True, True), (0.0, True, False), (-3.0, True, False), (np.nan, False, False)]:
        rec = FK.records([base], [5], [score])
        fr, out, drawn = one_frame(L, W, Hh, "gray", rec, un)
        assert drawn == int(with_flag), score
        _, _, drawn2 = one_frame(L, W, Hh, "gray", rec, st)
        assert drawn2 == int(without), score
        if with_flag and not without:   # an unmatched record: its own outline colour, the dot, no label
            vals = set(np.unique(fr.view(0, out)))
            assert vals == {0, 77, 200}, vals
        if without:
            assert set(np.unique(fr.view(0, out))) == {0, 255, 200, 150}
    # UNMATCHED draws cube and axes of a matched record only
    cam = PS.camera(W, Hh)
    R, t = PS.pose(cam, 32, 24, 24, 20, 10, 0)
    full = AC.style(L, AC.ALL_FLAGS)
    for score in (1.0, 0.0):
        rec = AC.posed_record(cam, R, t, score=score)
        ok, s, _ = AC.host_setup(L, rec, full, W, Hh, cam)
        live = (s["seg"]["box"][:, 0] <= s["seg"]["box"][:, 2])
        assert ok and live[:5].all() and live[5:].all() == (score > 0) and live[5:].any() == (score > 0) and (s["n"] > 0) == (score > 0)


def test_a_glmatrix_that_is_not_finite_keeps_the_outline(L):
    W, Hh = 96, 80
    cam = PS.camera(W, Hh)
    R, t = PS.pose(cam, 48, 40, 36, 25, 30, 40)
    full = AC.style(L, AC.DRAW_FLAGS)
    rec = AC.posed_record(cam, R, t, template_id=3)
    for slot, bad in [(0, np.nan), (7, np.inf), (15, np.nan), (3, -np.inf)]:
        r = rec.copy()
        r["glMatrix"][slot] = bad
        ok, s, _ = AC.host_setup(L, r, full, W, Hh, cam)
        live = s["seg"]["box"][:, 0] <= s["seg"]["box"][:, 2]
        assert ok and live[:5].all() and not live[5:].any() and s["n"] == 1


def test_a_point_behind_the_camera_drops_its_segments_only(L):
    W, Hh = 96, 80
    cam = PS.camera(W, Hh)
    R, t = np.diag([1.0, -1.0, -1.0]), np.array([0.0, 0.0, 4.0])    # the marker faces the camera, +Z towards it
    rec = AC.posed_record(cam, R, t)
    st = AC.style(L, AC.CUBE | AC.AXES, cube_height=5.0, axis_length=3.0)   # the cube's top at camera z = -1, the Z tip at z = 1
    ok, s, _ = AC.host_setup(L, rec, st, W, Hh, cam)
    live = (s["seg"]["box"][:, 0] <= s["seg"]["box"][:, 2]).tolist()
    assert ok and live[5:9] == [True] * 4 and live[9:17] == [False] * 8 and live[17:20] == [True] * 3
    st.axis_length = 4.0      # the Z tip at camera z = 0
    ok, s, _ = AC.host_setup(L, rec, st, W, Hh, cam)
    live = (s["seg"]["box"][:, 0] <= s["seg"]["box"][:, 2]).tolist()
    assert live[17:20] == [True, True, False]
    # the origin behind the camera: no axis at all; with nothing else asked for the record draws nothing
    rec2 = AC.posed_record(cam, R, np.array([0.0, 0.0, 4.0]))
    rec2["glMatrix"][14] = 1.0    # t.z = -1
    ok, s, box = AC.host_setup(L, rec2, AC.style(L, AC.AXES), W, Hh, cam)
    assert not ok and box[0] > box[2]


def test_a_bow_tie_is_its_four_edges(L):
    W, Hh = 64, 48
    c = np.array([[10, 8], [50, 40], [50, 8], [10, 40]], np.float64)
    st = AC.style(L, AC.OUTLINE, thickness=2, outline=(255, 255, 255, 255))
    fr, out, drawn = one_frame(L, W, Hh, "gray", FK.records([c.reshape(8)]), st)
    mask = fr.view(0, out)[..., 0] == 255
    d = np.min([AC.np_distance(W, Hh, c[k], c[(k + 1) % 4]) for k in range(4)], axis=0)
    assert drawn == 1 and mask[d <= 0.9].all() and not mask[d >= 1.1].any()
    assert mask[24, 30] and mask[8, 30] == False and mask[20, 50]   # noqa: E712  (the crossing; no edge 0 -- 2; the edge 1 -- 2)


def test_a_record_wholly_outside_draws_nothing(L):
    st = AC.style(L, AC.OUTLINE | AC.CORNER0 | AC.LABEL, thickness=16)
    for sq in (FK.axis_square(-60, 5, 30, 30), FK.axis_square(90, 5, 30, 30), FK.axis_square(5, -70, 30, 30), FK.axis_square(5, 80, 30, 30)):
        _, out, drawn = one_frame(L, 64, 48, "bgr", FK.records([sq]), st, fill=1)
        assert drawn == 0 and (out[FK.LEAD:-FK.LEAD] == 1).all()


# ---- pose primitives --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lens", [False, True])
def test_projected_axis_tips_and_cube_corners(L, lens):
    W, Hh = 640, 480
    specs = [(200, 160, 120, 40, 25, 30, 2, None), (450, 300, 90, 60, 200, 110, 2, None), (320, 400, 60, 0, 80, 0, 2, None)]
    sc = PS.scene("annotate", "lens" if lens else "pinhole", W, Hh, specs, lens=lens)
    assert any(sc.cam.distCoeffs) == lens
    st = AC.style(L, AC.CUBE | AC.AXES, axis_length=1.3, cube_height=0.8, thickness=1)
    tol = 1 / 32 + 1e-6    # the rounding to 1/16 px moves a coordinate by at most 1/32
    for m in sc.markers:
        rec = AC.posed_record(sc.cam, m.R, m.t)
        Rb, tb = PS.pose_of_glmatrix(rec["glMatrix"])
        assert np.abs(Rb - m.R).max() < 1e-12 and np.abs(tb - m.t).max() < 1e-12
        assert np.abs(rec["square"].reshape(4, 2) - m.quad).max() < 1e-4
        ok, s, _ = AC.host_setup(L, rec, st, W, Hh, sc.cam)
        assert ok
        seg = s["seg"]
        live = seg["box"][:, 0] <= seg["box"][:, 2]
        base = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64)
        top = base + [0, 0, 0.8]
        pts = AC.project3(sc.cam, m.R, m.t, np.concatenate([base, top, [[0, 0, 0], [1.3, 0, 0], [0, 1.3, 0], [0, 0, 1.3]]]))
        want = {}
        for e in range(4):
            want[5 + e] = (pts[e], pts[(e + 1) % 4])
            want[9 + e] = (pts[4 + e], pts[4 + (e + 1) % 4])
            want[13 + e] = (pts[e], pts[4 + e])
        for i in range(3):
            want[17 + i] = (pts[8], pts[9 + i])
        for p, (a, b) in want.items():
            if not live[p]:     # only a segment whose grown box misses the frame may be absent
                assert max(a[0], b[0]) < -0.5 or max(a[1], b[1]) < -0.5 or min(a[0], b[0]) > W - 0.5 or min(a[1], b[1]) > Hh - 0.5, p
                continue
            assert np.abs(seg[p]["a"] / 16.0 - a).max() <= tol and np.abs(seg[p]["b"] / 16.0 - b).max() <= tol, (p, seg[p], a, b)
        assert live[5:].sum() >= 12
        # the cube's base coincides with the projection of the model rectangle, the record's own square
        for e in range(4):
            assert np.abs(seg[5 + e]["a"] / 16.0 - m.quad[e]).max() <= tol + 1e-4
        assert [int(c) for c in seg["rgba"][17:20]] == [AC.rgba_word(c) for c in ((255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255))]


def test_the_cube_stands_on_the_side_the_z_axis_points_to(L):
    W, Hh = 200, 160
    cam = PS.camera(W, Hh)
    R, t = PS.pose(cam, 100, 80, 50, 35, 15, 60)
    rec = AC.posed_record(cam, R, t, ratio=1.5)
    st = AC.style(L, AC.CUBE | AC.AXES, axis_length=0.7, cube_height=0.7)
    ok, s, _ = AC.host_setup(L, rec, st, W, Hh, cam)
    assert ok
    tops = np.array([s["seg"][13 + e]["b"] for e in range(4)]) / 16.0
    z_tip = s["seg"][19]["b"] / 16.0
    # the diagonals of the top meet at the projection of its centre (0, 0, 0.7): the Z axis' tip
    p0, p1, p2, p3 = tops
    lam = np.linalg.solve(np.stack([p2 - p0, p1 - p3], axis=1), p1 - p0)[0]
    assert np.abs(p0 + lam * (p2 - p0) - z_tip).max() < 0.25
    bases = np.array([s["seg"][5 + e]["a"] for e in range(4)]) / 16.0
    want = AC.project3(cam, R, t, [[-1.5, -1, 0], [1.5, -1, 0], [1.5, 1, 0], [-1.5, 1, 0]])
    assert np.abs(bases - want).max() <= 1 / 32 + 1e-6       # the aspect ratio is the record's


# ---- label ------------------------------------------------------------------------------------------------------------------------

def label_mask(L, W, Hh, square, tid, scale, fmt="gray"):
    st = AC.style(L, AC.LABEL, label_scale=scale, label=(255, 255, 255, 255))
    fr, out, drawn = one_frame(L, W, Hh, fmt, FK.records([square], [tid]), st)
    return fr.view(0, out)[..., 0] == 255, drawn


def test_every_glyph_is_the_font_table(L):
    for d in range(10):
        bits = L.annotate_glyph_emul(d)
        table = np.array([[(bits >> (5 * r + 4 - c)) & 1 for c in range(5)] for r in range(7)], bool)
        assert (table == AC.glyph(d)).all(), d
        mask, drawn = label_mask(L, 32, 24, FK.axis_square(10, 8, 9, 9), d, 1)   # centre (14, 12): columns 12 .. 16, rows 9 .. 15
        want = np.zeros((24, 32), bool)
        want[9:16, 12:17] = AC.glyph(d)
        assert drawn == 1 and (mask == want).all(), d


@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("number", [0, 7, 10, 4095])
def test_labels_of_several_digits_are_centred(L, number, scale):
    W, Hh = 240, 120
    cx, cy = 120.0, 60.0
    mask, drawn = label_mask(L, W, Hh, [cx - 30, cy - 20, cx + 30, cy - 20, cx + 30, cy + 20, cx - 30, cy + 20], number, scale)
    pic = AC.label_picture(number, scale)
    lh, lw = pic.shape
    assert lw == (6 * len(str(number)) - 1) * scale and lh == 7 * scale
    ox, oy = int(np.rint(cx - (lw - 1) / 2)), int(np.rint(cy - (lh - 1) / 2))
    want = np.zeros((Hh, W), bool)
    want[oy:oy + lh, ox:ox + lw] = pic
    assert drawn == 1 and (mask == want).all()
    ys, xs = np.nonzero(mask)
    assert abs((xs.min() + xs.max()) / 2 - cx) <= 0.5 + (scale if number in (7, 10) else 0) and abs((ys.min() + ys.max()) / 2 - cy) <= 0.5


def test_the_automatic_scale_follows_the_shorter_side_and_clamps(L):
    st = AC.style(L, AC.LABEL, label_scale=0)
    for side, want in [(5, 1), (23.9, 1), (47.9, 1), (48, 2), (71.9, 2), (72, 3), (191.9, 7), (192, 8), (1000, 8)]:
        sq = [100, 100, 100 + 4 * side, 100, 100 + 4 * side, 100 + side, 100, 100 + side]
        ok, s, _ = AC.host_setup(L, FK.records([sq], [42])[0], st, 4000, 1400)
        assert ok and s["scale"] == want and s["n"] == 2 and s["digit"][:2].tolist() == [4, 2], (side, s["scale"])
    # a negative template id has no label
    ok, s, _ = AC.host_setup(L, FK.records([FK.axis_square(10, 10, 50, 50)], [-1])[0], st, 100, 100)
    assert not ok and s["n"] == 0


def test_a_label_cut_by_each_edge_of_the_frame(L):
    W, Hh = 60, 40
    pic = AC.label_picture(4095, 2)     # 46 x 14
    lh, lw = pic.shape
    for cx, cy in [(3.0, 20.0), (57.0, 20.0), (30.0, 2.0), (30.0, 38.0), (1.0, 1.0), (59.0, 39.0)]:
        mask, drawn = label_mask(L, W, Hh, [cx - 5, cy - 5, cx + 5, cy - 5, cx + 5, cy + 5, cx - 5, cy + 5], 4095, 2)
        ox, oy = int(np.rint(cx - (lw - 1) / 2)), int(np.rint(cy - (lh - 1) / 2))
        big = np.zeros((Hh + 2 * lh, W + 2 * lw), bool)
        big[oy + lh:oy + 2 * lh, ox + lw:ox + 2 * lw] = pic
        want = big[lh:lh + Hh, lw:lw + W]
        assert drawn == 1 and (mask == want).all() and want.any() and want.sum() < pic.sum(), (cx, cy)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_the_style_validator(L):
    bad = L.annotate_style_bad_emul
    st = AC.style(L)
    assert st.flags == AC.OUTLINE | AC.CORNER0 | AC.LABEL and st.thickness == 2 and st.label_scale == 0
    assert (st.axis_length, st.cube_height) == (1.0, 1.0) and list(st.outline) == [0, 255, 0, 255]
    assert bad(C.byref(st), 0) == 0 and bad(C.byref(st), 1) == 0
    assert bad(None, 1) != 0
    cases = [dict(thickness=0), dict(thickness=17), dict(thickness=-1), dict(label_scale=-1), dict(label_scale=9),
             dict(axis_length=-0.5), dict(axis_length=math.nan), dict(axis_length=math.inf), dict(cube_height=-1e-300),
             dict(cube_height=math.nan), dict(cube_height=-math.inf), dict(flags=128 | AC.OUTLINE), dict(flags=-1), dict(flags=1 << 30 | 1),
             dict(flags=0), dict(flags=AC.UNMATCHED), dict(flags=AC.COLOR_BY_TEMPLATE), dict(flags=AC.UNMATCHED | AC.COLOR_BY_TEMPLATE)]
    for kw in cases:
        assert bad(C.byref(AC.style(L, **kw)), 1) != 0, kw
    for kw in [dict(thickness=1), dict(thickness=16), dict(label_scale=8), dict(axis_length=0.0), dict(cube_height=1e300), dict(flags=AC.ALL_FLAGS)]:
        assert bad(C.byref(AC.style(L, **kw)), 1) == 0, kw
    for flags in (AC.AXES, AC.CUBE, AC.ALL_FLAGS):
        assert bad(C.byref(AC.style(L, flags)), 0) != 0 and bad(C.byref(AC.style(L, flags)), 1) == 0
    for flags in (AC.OUTLINE, AC.CORNER0, AC.LABEL):
        assert bad(C.byref(AC.style(L, flags)), 0) == 0


# ---- sanitizers -------------------------------------------------------------------------------------------------------------------

def test_stand_alone_program_under_the_sanitizers():
    """tests/emul/annotate_emul.cpp with its own main, built with -fsanitize=address,undefined and run as a program: frames 1x1, 3x2,
    257x17 and 70x37 in every format on heap blocks of exactly their size, records at, on and beyond every edge, thickness 16 at a
    corner, coordinates at and beyond the clamp range"""
    run_sanitized("annotate_emul", "ANNOTATE_EMUL_MAIN", "bytes changed", timeout=600)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------

def test_abi_surface(L):
    """the three entry points are declared in the header and exported by the built library; the style's size and defaults, the
    module's names"""
    import opencv_ar_amd as oa
    header = open(os.path.join(H.ROOT, "include", "ocvar_hip.h")).read()
    lib = oa.hip_lib()
    for name in ("ocvar_hip_annotate_default_style", "ocvar_hip_annotate", "ocvar_hip_annotate_records"):
        assert re.search(r"\bint %s\(" % name, header) and name in oa.HIP_SYMBOLS and hasattr(lib, name), name
    assert "/* 56 bytes */" in header and C.sizeof(oa.AnnotateStyle) == C.sizeof(AC.Style) == 56
    for k, name in enumerate(["OUTLINE", "CORNER0", "AXES", "CUBE", "LABEL", "UNMATCHED", "COLOR_BY_TEMPLATE"]):
        assert re.search(r"OCVAR_ANNO_%s = %d\b" % (name, 1 << k), header) and getattr(oa, "ANNO_" + name) == 1 << k
    assert re.search(r"OCVAR_ANNO_RECORD_BYTES = 696\b", header) and oa.ANNO_RECORD_BYTES == 696 == AC.REC_DTYPE.itemsize + 16
    assert re.search(r"OCVAR_ANNO_MAX_COORD = %d\b" % AC.MAX_COORD, header) and oa.ANNO_MAX_COORD == AC.MAX_COORD
    # the library's default style is the core's
    a, b = oa.AnnotateStyle(), AC.Style()
    assert lib.ocvar_hip_annotate_default_style(C.byref(a)) == 0 and lib.ocvar_hip_annotate_default_style(None) == FK.E_ARG
    L.annotate_default_style_emul(C.byref(b))
    assert bytes(a) == bytes(b)
    # sizeof(OcvarAnnotateStyle) as the built library has it: it writes exactly 56 bytes
    block = (C.c_uint8 * 80)(*([0xA5] * 80))
    assert lib.ocvar_hip_annotate_default_style(C.byref(block, 8)) == 0
    assert bytes(block[8:64]) == bytes(b) and set(block[:8]) | set(block[64:]) == {0xA5}
    # annotate_style
    s = oa.annotate_style()
    assert bytes(s) == bytes(b)
    s = oa.annotate_style(axes=True, cube=True, label=False, thickness=5, label_scale=3, axis_length=2, cube_height=0.5, outline_color=(1, 2, 3, 4),
                          unmatched=True, color_by_template=True, label_color=(9, 8, 7, 6))
    assert s.flags == AC.ALL_FLAGS & ~AC.LABEL and (s.thickness, s.label_scale, s.axis_length, s.cube_height) == (5, 3, 2.0, 0.5)
    assert list(s.outline) == [1, 2, 3, 4] and list(s.label) == [9, 8, 7, 6] and list(s.cube) == list(b.cube)
    for kw in [dict(thickness=0), dict(thickness=17), dict(thickness=2.0), dict(label_scale=9), dict(axis_length=-1), dict(cube_height=math.nan),
               dict(outline_color=(1, 2, 3)), dict(outline_color=(1, 2, 3, 256)), dict(colour=1), dict(outline=False, corner0=False, label=False)]:
        with pytest.raises(ValueError):
            oa.annotate_style(**kw)
    assert lib.ocvar_hip_annotate(None, None, 0, 0, 0, 0, 0, None, None) == FK.E_ARG
    assert lib.ocvar_hip_annotate_records(None, None, 0, 0, 0, 0, 0, 0, None, None, 0, None, None) == FK.E_ARG

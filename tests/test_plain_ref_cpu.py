"""CPU tests: the oracle's image, contour and polygon stages against tests/plain_ref.py, a second reference written from SURVEY.md
Appendix A and from the topological definition of a border by other means (scipy filters, connected-component labels, rationals).
Every comparison is exact.  A contour in which the plain reference meets a knife edge (plain_ref.approx) is left out of the
comparison of polygons and squares, never counted as equal, and how many there may be is bounded."""
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import plain_ref as R
import plain_ref_scenes as PS
import work_cut_scenes as S
from border_shapes import sawtooth_frame
from follow_limit_scenes import parity_frames
from helpers import P
from test_starts_cpu import build_lib

BIN_SIZES = [(16, 16), (17, 19), (18, 16), (33, 47), (64, 80), (121, 97), (240, 320), (496, 270)]   # width x height


def binarise_inputs(w, h):
    """the grey images of one size: noise, smooth, 4x4 blocks, a dark rectangle, a textured frame with markers"""
    rng = np.random.default_rng(w * 1000 + h)
    ys, xs = np.mgrid[0:h, 0:w]
    smooth = (127 + 90 * np.sin(xs / 7.0) * np.cos(ys / 5.0) + rng.integers(-3, 4, (h, w))).astype(np.uint8)
    rect = np.full((h, w), 210, np.uint8)
    rect[h // 4:h - h // 5, w // 5:w - w // 4] = 30
    side = min(w, h) - 8
    return {"noise": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "smooth": smooth,
            "blocks": np.kron(rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), np.int64))[:h, :w].astype(np.uint8),
            "rectangle": rect,
            "markers": np.ascontiguousarray(S.frame_of(w, h, w + h, [(4, 4, side // 2), (w - side // 2 - 3, h - side // 2 - 3, side // 2)])[..., 0])}


def oracle_planes(g):
    g = np.ascontiguousarray(g)
    h, w = g.shape
    b, up = np.zeros((h & -2, w & -2), np.uint8), np.zeros((h & -2, w & -2), np.uint8)
    H.oracle().orc_binarise(P(g), w, h, w, P(b), P(up))
    return b, up


@pytest.mark.parametrize("w,h", BIN_SIZES)
def test_binarise_equals_the_plain_reference(w, h):
    for name, g in binarise_inputs(w, h).items():
        b, up = R.binarise(g)
        ob, oup = oracle_planes(g)
        assert np.array_equal(H.oracle_binarise(g), ob)
        assert np.array_equal(oup, up), ("pyrUp plane", name, w, h, int((oup != up).sum()))
        assert np.array_equal(ob, b), ("threshold plane", name, w, h, int((ob != b).sum()))


# ---- the binary images whose borders are compared ------------------------------------------------------------------------------
N_RANDOM = 1000


def random_binaries():
    """seeded binary images with sides 5 .. 39 at densities 0.3, 0.5, 0.7 and 0.85, every fifth one in 3x3 blocks"""
    rng = np.random.default_rng(20240611)
    for k in range(N_RANDOM):
        h, w = (int(v) for v in rng.integers(5, 40, 2))
        d = (0.3, 0.5, 0.7, 0.85)[k % 4]
        if k % 5 == 0:
            b = np.kron(rng.random(((h + 2) // 3, (w + 2) // 3)) < d, np.ones((3, 3), bool))[:h, :w]
        else:
            b = rng.random((h, w)) < d
        yield "random_%d" % k, b.astype(np.uint8) * 255


def drawn_binaries():
    """the binarised fixed scenes, sawtoothed borders, and 320x240 windows of the 1080p noise and the 4K capacity frame"""
    for W, Hh in PS.SIZES:
        yield "scene_%dx%d" % (W, Hh), PS.scene(W, Hh).binary
    yield "sawtooth_4", R.binarise(sawtooth_frame(320, 240, 4, [(12, 12, 308, 132), (20, 148, 140, 228), (170, 150, 300, 226)])[..., 0])[0]
    yield "sawtooth_2", R.binarise(sawtooth_frame(320, 240, 2, [(20, 20, 300, 220)])[..., 0])[0]
    big = parity_frames()
    yield "noise_window", R.binarise(big["noise"][400:640, 700:1020, 0])[0]
    yield "capacity_window", R.binarise(big["capacity"][0:240, 0:320, 0])[0]
    yield "capacity_corner", R.binarise(big["capacity"][1960:2160, 3520:3840, 0])[0]


class Corpus:
    """every input with the plain reference's trace of it, made once"""

    def __init__(self):
        self.items = [(name, b, R.trace(b)) for gen in (random_binaries(), drawn_binaries()) for name, b in gen]
        self.polygons, self._borders = {}, {}

    def borders(self, name, b):
        if name not in self._borders:
            self._borders[name] = R.borders(b)
        return self._borders[name]

    def polygon(self, name, k, pts):
        if (name, k) not in self.polygons:
            self.polygons[(name, k)] = R.polygon_of(pts)
        return self.polygons[(name, k)]


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


def test_contours_equal_the_plain_walk(corpus):
    n = 0
    for name, b, tr in corpus.items:
        cs, starts, holes = H.oracle_contours(b)
        assert len(cs) == len(tr), (name, len(cs), len(tr))
        for k, ((pts, start, hole), c) in enumerate(zip(tr, cs)):
            assert (start, hole) == (starts[k], holes[k]), (name, k)
            assert pts.shape == c.shape and np.array_equal(pts, c), (name, k)
        assert all(one[1] > two[1] for one, two in zip(tr, tr[1:])), ("list order: strictly descending start", name)
        n += len(tr)
    print("borders compared with the oracle: %d in %d images" % (n, len(corpus.items)))
    assert n > 20000


def test_plain_walk_satisfies_the_labels_and_pick_s_theorem(corpus):
    """borders() knows nothing of walking: starts and hole flags are first pixels of components, the visited pixels those next
    to the component on the other side; and on an outer border that visits no pixel twice, the pixels on or inside it number
    |area| + B / 2 + 1"""
    n = simple = twice = 0
    for name, b, tr in corpus.items:
        want = corpus.borders(name, b)
        w = b.shape[1]
        assert {(s, h) for _, s, h in tr} == set(want) and len(tr) == len(want), name
        for pts, start, hole in tr:
            px = R.pixels_of(pts)
            visited, filled = want[(start, hole)]
            assert {y * w + x for x, y in px} == visited, (name, start, hole)
            if len(set(px)) != len(px):
                twice += 1
            elif not hole:
                assert filled == abs(R.area(pts)) + Fraction(R.lattice_points_on(pts), 2) + 1, (name, start)
                simple += 1
            n += 1
    print("borders checked against labels: %d, Pick's theorem on %d, %d visit a pixel twice" % (n, simple, twice))
    assert simple > 3000 and twice > 1000


# ---- primitives ----------------------------------------------------------------------------------------------------------------
def oracle_primitives(pts):
    """(arc length, polygon at 0.02 of it, area, convex) of a contour, by the oracle"""
    p = np.ascontiguousarray(pts, np.int32).reshape(-1, 2)
    n = len(p)
    o = H.oracle()
    assert o.orc_get_approx_variant() == 0
    arc = o.orc_arc_length_closed(P(p), n)
    out = np.zeros((n + 1, 2), np.int32)
    m = o.orc_approx_poly(P(p), n, arc * 0.02, P(out))
    return arc, out[:m].copy(), o.orc_contour_area(P(p), n), bool(o.orc_is_convex(P(p), n))


def check_primitives(pts, polygon=None, where=None):
    """the oracle's primitives on a contour and on its polygon against the plain ones; returns True when the polygon was
    compared (no knife edge)"""
    arc, poly, a, convex = oracle_primitives(pts)
    assert arc == R.arc_length(pts), ("arc length", where)
    assert Fraction(a) == abs(R.area(pts)), ("area", where)
    assert convex == R.is_convex(pts), ("convexity", where)
    want, knife = polygon if polygon is not None else R.polygon_of(pts)
    if knife:
        return False
    assert poly.shape == want.shape and np.array_equal(poly, want), ("polygon", where, poly.tolist(), want.tolist())
    if len(want):
        _, _, a, convex = oracle_primitives(want)
        assert Fraction(a) == abs(R.area(want)) and convex == R.is_convex(want), ("area / convexity of the polygon", where)
    return True


def test_primitives_on_every_contour(corpus):
    n = undecided = n_random = undecided_random = 0
    for name, b, tr in corpus.items:
        for k, (pts, start, hole) in enumerate(tr):
            if len(pts) < 4:
                continue
            ok = check_primitives(pts, corpus.polygon(name, k, pts), (name, k))
            n += 1
            undecided += not ok
            if name.startswith("random"):
                n_random += 1
                undecided_random += not ok
            else:
                assert ok, ("a knife edge in a fixed input", name, k)
    print("contours of >= 4 points compared: %d (%d of random images); undecided: %d" % (n, n_random, undecided))
    assert n_random > 5000 and undecided_random * 1000 <= n_random


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]


def sawtooth(n, tooth=2):
    """a closed strip whose upper edge is a sawtooth of `tooth` pixels, n teeth"""
    top = [(tooth * k, 0 if k % 2 == 0 else tooth) for k in range(2 * n + 1)]
    return top[::-1] + [(0, 4 * tooth + n), (2 * tooth * n, 4 * tooth + n)]


HAND_MADE = {
    "rectangle": rect(3, 4, 40, 30), "thin rectangle": rect(0, 0, 200, 3), "square": rect(10, 10, 33, 33),
    "unit square": rect(0, 0, 1, 1), "large rectangle": rect(5, 7, 30000, 20000),
    "rhombus": [(20, 0), (0, 12), (20, 24), (40, 12)], "flat rhombus": [(60, 0), (0, 5), (60, 10), (120, 5)],
    "rhombus with stepped sides": [(20, 0), (10, 6), (9, 7), (0, 12), (10, 18), (20, 24), (31, 18), (40, 12), (30, 6)],
    "L": [(0, 0), (0, 40), (30, 40), (30, 28), (12, 28), (12, 0)],
    "U": [(0, 0), (0, 40), (36, 40), (36, 0), (26, 0), (26, 30), (10, 30), (10, 0)],
    "sawtooth": sawtooth(12), "long sawtooth": sawtooth(60), "sawtooth of 1": sawtooth(9, 1),
    "quad with a reflex vertex": [(0, 0), (10, 20), (0, 40), (50, 20)],
    "4-gon with three collinear vertices": [(0, 0), (0, 30), (30, 30), (15, 15)],
    "4-gon with a collinear vertex on an axis": [(0, 0), (0, 30), (15, 30), (30, 30)],
    "quad, clockwise": [(0, 0), (40, 0), (40, 30), (0, 30)],
    "nearly collinear vertex": [(0, 0), (0, 60), (100, 61), (200, 60), (200, 0)],
    "two vertices the clean-up pass drops": [(0, 0), (3, 50), (0, 100), (50, 103), (100, 100), (97, 50), (100, 0), (50, 3)],
    "one point": [(5, 5)], "two points": [(5, 5), (9, 5)], "two points, diagonal": [(5, 5), (25, 25)],
    "three points": [(0, 0), (0, 30), (40, 0)], "three collinear points": [(0, 0), (10, 10), (20, 20)],
    "there and back": [(0, 0), (30, 0), (60, 0), (30, 0)],
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_primitives_on_hand_made_contours(name):
    pts = np.array(HAND_MADE[name], np.int64)
    for eps_pts in (pts, pts[::-1].copy(), np.roll(pts, 1, axis=0), pts + 1000):
        assert check_primitives(eps_pts, where=name), ("a knife edge in a hand-made contour", name)
    # and at accuracies from none to more than the contour's size
    p32 = np.ascontiguousarray(pts, np.int32)
    for eps in (0.0, 0.5, 1.0, 2.0, 3.5, 7.0, 1e3, 1e9):
        out = np.zeros((len(pts) + 1, 2), np.int32)
        m = H.oracle().orc_approx_poly(P(p32), len(p32), eps, P(out))
        want, knife = R.approx(pts, eps)
        assert knife or np.array_equal(out[:m], want), (name, eps, out[:m].tolist(), want.tolist())


def test_what_the_special_cases_are():
    assert not R.is_convex(HAND_MADE["quad with a reflex vertex"])
    assert not R.is_convex(HAND_MADE["4-gon with three collinear vertices"]) and not R.is_convex(HAND_MADE["4-gon with a collinear vertex on an axis"])
    assert R.is_convex(HAND_MADE["quad, clockwise"]) and R.is_convex(HAND_MADE["quad, clockwise"][::-1])
    assert not any(R.is_convex(HAND_MADE[k]) for k in ("one point", "two points", "three collinear points")) and R.is_convex(HAND_MADE["three points"])
    assert R.area(HAND_MADE["quad, clockwise"]) == -R.area(HAND_MADE["quad, clockwise"][::-1]) == 1200
    assert R.arc_length(HAND_MADE["one point"]) == 0 and R.arc_length(HAND_MADE["two points"]) == 8
    assert len(R.polygon_of(HAND_MADE["two vertices the clean-up pass drops"])[0]) < 8


# ---- squares -------------------------------------------------------------------------------------------------------------------
def check_squares(g, where, want=None):
    sq, starts, undecided = want if want is not None else R.find_squares(g)
    got = H.oracle_find_squares(g)
    assert not undecided, ("a knife edge in a fixed scene", where)
    assert got.shape == sq.shape and np.array_equal(got, sq), ("squares", where, got.tolist(), sq.tolist())
    return len(sq)


def test_squares_of_the_fixed_scenes_and_of_synthetic_frames():
    n = 0
    for W, Hh in PS.SIZES:
        sc = PS.scene(W, Hh)
        n += check_squares(sc.grey, (W, Hh), sc.squares)
    assert n > 50
    for config in (1, 2):
        cfg = H.synth_config(config)
        for f in range(8):
            g = R.grey(H.synth_frame(cfg, f)[0], "bgr")
            assert check_squares(g, (config, f)) > 0


def test_crop_squares_of_the_fixed_scenes():
    """the crop pass's squares: find_squares of the oracle on the plain reference's grey crops"""
    n = 0
    for W, Hh in ((320, 240), (496, 270)):
        sc = PS.scene(W, Hh)
        for q in sc.squares[0]:
            x0, y0, w, h = R.crop_rect(q, W, Hh)
            assert 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= Hh
            n += check_squares(sc.grey[y0:y0 + h, x0:x0 + w], (W, Hh, q.tolist()))
    assert n > 20


def test_what_the_fixed_scenes_are_there_for():
    """both sides of the area cut and the cut itself, both sides of the border rule, a reflex 4-gon, a border that visits a pixel
    twice: on the plain reference, so that a changed scene that loses one fails here"""
    areas, first_x, reflex, twice, on_the_cut = [], {}, 0, 0, 0
    for W, Hh in PS.SIZES:
        sc = PS.scene(W, Hh)
        kept = {tuple(q.ravel().tolist()) for q in sc.squares[0]}
        for (pts, start, hole), (poly, knife) in zip(sc.contours, sc.polygons):
            assert not knife
            px = R.pixels_of(pts)
            twice += len(set(px)) != len(px)
            if len(poly) != 4:
                continue
            a = abs(R.area(poly))
            if R.is_convex(poly):
                areas.append(a)
                on_the_cut += a == 500 and 2 < poly[0][0] < W - 2 and 2 < poly[0][1] < Hh - 2
            elif a > 500:
                reflex += 1
            if a > 500 and R.is_convex(poly) and 2 < poly[0][1] < Hh - 2:
                x = int(poly[0][0])
                side = x if x <= 3 else x - W
                assert (tuple(poly.ravel().tolist()) in kept) == (2 < x < W - 2)
                first_x[side] = first_x.get(side, 0) + 1
        if (W, Hh) in ((320, 240), (496, 270)):
            assert "neck" in sc.names and "dart" in sc.names and "rings" in sc.names and "solid_32" in sc.names
    assert any(400 < a <= 500 for a in areas) and any(500 < a <= 600 for a in areas), sorted(float(a) for a in areas)
    # (where a rounded corner of a drawn square lands depends on the frame's noise: the four cases are asked of the scenes together)
    assert all(first_x.get(k) for k in (2, 3, -3, -2)), ("vertex 0 either side of the border rule", {k: first_x.get(k) for k in (2, 3, -3, -2)})
    assert on_the_cut >= 2, "a convex 4-gon of area 500 exactly, which only the area rule drops"
    assert reflex >= 2 and twice >= 10, (reflex, twice)
    assert "blocks" in PS.scene(320, 240).names


# ---- the device's border-start rule ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def starts_lib():
    return build_lib()


def test_start_rule_lists_every_start_of_the_labels(corpus, starts_lib):
    """the pixel-local rule of starts_core.h lists the first pixel of every component with its hole flag (and more: it cannot see
    whether a pixel is its component's first).  A hole's start is the hole's own first pixel -- the scan position, as the
    oracle's `starts` have it --, not the pixel before it that A.5 begins the walk on."""
    n = extra = 0
    for name, b, tr in corpus.items:
        z = np.ascontiguousarray(R.framed(b) * 255)
        out = np.zeros(z.size + 1, np.uint32)
        k = starts_lib.se_rule(P(z), z.shape[1], z.shape[0], P(out), out.size)
        assert 0 <= k <= out.size
        listed = set(out[:k].tolist())
        want = {s | h << 31 for s, h in corpus.borders(name, b)}
        assert want <= listed, (name, sorted(want - listed)[:8])
        n += len(want)
        extra += len(listed) - len(want)
    print("starts the rule must list: %d; it lists %d more" % (n, extra))
    assert n > 20000

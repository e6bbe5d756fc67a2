"""The fixed scenes of tests/test_plain_ref_cpu.py and tests/test_gpu_plain_ref.py: one frame per size, at the smallest sizes that
reach each way the frame kernel cuts its work.  Every scene is a textured background with drawn markers
(work_cut_scenes.frame_of) that also holds, drawn here in numpy, as many of these as fit, in this order: solid squares of sides
26 .. 32 (after the binarise's erosion their inner islands lie on both sides of the area cut at 500), a quad whose polygon has
area 500 exactly, light squares
against the left edge and dark kites against the right one (both sides of the border rule on vertex 0), nested rings, a tilted quad, a rhombus, a
non-convex 4-gon, two blobs joined by a thin neck (a border that visits a pixel twice) and, at 320x240 only, a patch of 4x4
block noise.  What the scenes are there for is asserted on the plain reference (tests/test_plain_ref_cpu.py), not assumed."""
import numpy as np

import plain_ref as R
import work_cut_scenes as S

DARK, LIGHT = 20, 235
# width x height: 16x16 and 18x16 the API's minimum; 17x19 and 67x51 odd sides (the even ROI, the unread last row and column);
# 242, 244 and 256 wide: a last strip of 2, 4 and 16 columns after MARCH_STRIP = 240; 241 and 481 wide: an odd width whose last
# column begins a grey panel; 496x270: three strips, two chunks, a seam row; 320x240
SIZES = [(16, 16), (18, 16), (17, 19), (67, 51), (242, 48), (244, 48), (256, 48), (241, 40), (481, 40), (496, 270), (320, 240)]
FORMATS = ("bgr", "rgb", "bgra", "rgba", "gray")


def _polygon(h, w, pts):
    """mask [h, w] of the pixels inside a convex polygon given clockwise on the screen"""
    y, x = np.mgrid[0:h, 0:w]
    m = np.ones((h, w), bool)
    for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
        m &= (x1 - x0) * (y - y0) - (y1 - y0) * (x - x0) >= 0
    return m


def _solid(side):
    def draw():
        p = np.full((side + 10, side + 10), LIGHT, np.uint8)
        p[5:5 + side, 5:5 + side] = DARK
        return p
    return draw


def _light_square(side, lead):
    """a light square inside a dark line 4 pixels wide on a light patch, `lead` columns of the line to its left"""
    def draw():
        p = np.full((side + 16, side + lead + 8), LIGHT, np.uint8)
        p[4:12 + side, 0:lead + side + 4] = DARK
        p[8:8 + side, lead:lead + side] = LIGHT
        return p
    return draw


def _dark_kite(beyond):
    """a dark kite pointing right on a light patch that ends `beyond` columns behind its tip: the hole border around it starts
    its polygon at the tip"""
    def draw():
        h, w = 44, 51 + beyond
        p = np.full((h, w), LIGHT, np.uint8)
        p[_polygon(h, w, [(36, 6), (50, 21), (36, 36), (6, 21)])] = DARK
        return p
    return draw


def _area_500():
    """a dark quad whose hole border becomes a convex 4-gon of area 500 exactly: the area rule's own edge (found by search)"""
    p = np.full((48, 52), LIGHT, np.uint8)
    p[_polygon(48, 52, [(12, 12), (37, 14), (40, 34), (15, 32)])] = DARK
    return p


def _rings():
    p = np.full((52, 52), LIGHT, np.uint8)
    for k, v in ((4, DARK), (11, LIGHT), (18, DARK), (23, LIGHT)):
        p[k:52 - k, k:52 - k] = v
    return p


def _tilted():
    p = np.full((60, 60), LIGHT, np.uint8)
    p[_polygon(60, 60, [(14, 6), (53, 16), (44, 54), (6, 42)])] = DARK
    return p


def _rhombus():
    y, x = np.mgrid[0:52, 0:72]
    p = np.full((52, 72), LIGHT, np.uint8)
    p[np.abs(x - 36) * 20 + np.abs(y - 26) * 30 <= 600] = DARK
    return p


def _dart():
    """a dark square with its far corner pushed in to the middle: the 4-gon (6, 6), (60, 6), (30, 30), (6, 60), reflex at (30, 30)"""
    p = np.full((68, 68), LIGHT, np.uint8)
    p[_polygon(68, 68, [(6, 6), (60, 6), (30, 30)]) | _polygon(68, 68, [(6, 6), (30, 30), (6, 60)])] = DARK
    return p


def _neck():
    p = np.full((40, 64), DARK, np.uint8)
    p[8:32, 6:28] = LIGHT
    p[8:32, 36:58] = LIGHT
    p[19:21, 28:36] = LIGHT
    return p


def _blocks():
    rng = np.random.default_rng(404)
    return np.kron(rng.integers(0, 2, (12, 16)) * 255, np.ones((4, 4), np.int64)).astype(np.uint8)


def _place(img, used, patch, x=None):
    """put a patch at the first free place in raster order on a grid of 4 pixels (x given: in that column); False if none"""
    h, w = patch.shape
    H, W = img.shape
    for y in range(0, H - h + 1, 4):
        for x0 in (range(0, W - w + 1, 4) if x is None else (x,)):
            if x0 < 0 or x0 + w > W or used[y:y + h, x0:x0 + w].any():
                continue
            img[y:y + h, x0:x0 + w] = patch
            used[y:y + h, x0:x0 + w] = True
            return True
    return False


def markers_of(W, H):
    """the drawn markers of a scene: (x, y, side)"""
    if W >= 320:
        return [(W - 72, H - 72, 64), (W - 132, H - 56, 48)]
    if H >= 40 and W >= 67:
        return [(W - 40, 4, H - 10)] if W < 100 else [(W - 44, 4, H - 10), (W // 2, 5, H - 12)]
    return []


_cache = {}


def grey_scene(W, H):
    """the grey image of the scene of one size, and the names of the drawn items that fitted"""
    if (W, H) in _cache:
        return _cache[(W, H)]
    marks = markers_of(W, H)
    g = np.ascontiguousarray(S.frame_of(W, H, 31 * W + H, marks)[..., 0])
    used = np.zeros((H, W), bool)
    for x, y, side in marks:
        used[max(y - 4, 0):y + side + 4, max(x - 4, 0):x + side + 4] = True
    items = []
    if W >= 160:
        # vertex 0 of the light squares' islands lands on x = 2 and 3; of the kites' hole borders, on W - 2 and W - 3 -- asserted
        items += [("left_%d" % x0, _light_square(30, x0), 0) for x0 in (3, 4)]
        if W % 2 == 0:
            items += [("right_%d" % t, _dark_kite(t), -1) for t in (1, 2)]
    items += [("solid_%d" % s, _solid(s), None) for s in range(26, 33)]
    items += [("area_500", lambda: _area_500(), None), ("rings", lambda: _rings(), None), ("tilted", lambda: _tilted(), None), ("rhombus", lambda: _rhombus(), None),
              ("dart", lambda: _dart(), None), ("neck", lambda: _neck(), None)]
    if (W, H) == (320, 240):
        items.append(("blocks", lambda: _blocks(), None))
    names = []
    for name, draw, x in items:
        patch = draw()
        if _place(g, used, patch, None if x is None else (0 if x == 0 else W - patch.shape[1])):
            names.append(name)
    _cache[(W, H)] = (g, names)
    return _cache[(W, H)]


def coloured(g, seed):
    """a BGR frame with unequal channels (an offset and noise of +-2 per channel) whose structure is that of grey image g"""
    r = np.random.default_rng(seed)
    c = g.astype(np.int64)[..., None] + np.array([-9, 4, -6]) + r.integers(-2, 3, g.shape + (3,))
    return np.clip(c, 0, 255).astype(np.uint8)


def in_format(bgr, fmt, seed=0):
    """the frame with the colours of a BGR frame in one of FORMATS (random alpha bytes; "gray": its grey image itself)"""
    if fmt == "gray":
        return R.grey(bgr, "bgr")
    alpha = np.random.default_rng(seed).integers(0, 256, bgr.shape[:2] + (1,), dtype=np.uint8)
    return np.ascontiguousarray({"bgr": bgr, "rgb": bgr[..., ::-1], "bgra": np.concatenate([bgr, alpha], 2),
                                 "rgba": np.concatenate([bgr[..., ::-1], alpha], 2)}[fmt])


_scenes = {}


class Scene:
    """the scene of one size: `bgr` the frame, `grey` its grey image by the plain reference, `names` the items drawn; binary,
    contours, squares and so on are computed when first asked for, once"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        g, self.names = grey_scene(W, H)
        self.bgr = coloured(g, 7 * W + H)
        self.grey = R.grey(self.bgr, "bgr")
        self._memo = {}

    def _get(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    @property
    def binary(self):
        return self._get("binary", lambda: R.binarise(self.grey)[0])

    @property
    def contours(self):
        return self._get("contours", lambda: R.trace(self.binary))

    @property
    def borders(self):
        return self._get("borders", lambda: R.borders(self.binary))

    @property
    def polygons(self):
        """(polygon, knife edge) of every contour, in list order"""
        return self._get("polygons", lambda: [R.polygon_of(c[0]) for c in self.contours])

    @property
    def squares(self):
        """R.find_squares of the grey image: (squares, their borders' start codes, undecided start codes)"""
        return self._get("squares", lambda: R.find_squares(self.grey, self.contours))


def scene(W, H):
    if (W, H) not in _scenes:
        _scenes[(W, H)] = Scene(W, H)
    return _scenes[(W, H)]


def variants(sc):
    """four distinct frames of a scene's size for a batch: the scene, mirrored left to right, upside down, and noise"""
    rng = np.random.default_rng(sc.W * 1000 + sc.H)
    return [sc.bgr, np.ascontiguousarray(sc.bgr[:, ::-1]), np.ascontiguousarray(sc.bgr[::-1]),
            rng.integers(0, 256, sc.bgr.shape, dtype=np.uint8)]

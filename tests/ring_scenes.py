"""Scenes for tests/test_gpu_rings.py and tests/test_rings_cpu.py: the verdicts of follow.hip::ring_quads_kernel -- whether the ring
of pixels next to the zeroed 1-px frame of a frame's or a crop's binary image is all set -- at every position of a hole and every
shape of ROI at which the kernel takes another path.  A frame is a flat light field of 235 with dark rectangles of 20; a ring is
opened by a dark dot of 1 x 1 or 2 x 2 pixels at or next to the ring pixel that is to go, found here by trying the dots on the
oracle's binarise: the dot must clear the target, at most 5 ring pixels in all, none further than 3 px from the target.  (The
binarise smooths over 2 x 2 blocks: such a dot takes a ring pixel with an odd coordinate only together with a neighbour, and the
neighbour of column 15 lies in the next tile or under another bit of the same mask.  So a few more frames and crops lose column 15
of the top row, or row 13 of the left column, alone -- to a dot of up to 3 x 3 below or beside it.)  The CPU test
asserts from the oracle alone that every scene reaches what it names; the GPU test compares the kernel's verdicts with `rule`
on the planes the same batch wrote.

Ring items are counted as the kernel counts them (ring_items): tiles = ns >> 4; items 0 .. 2 tiles - 1 are the 16-column tiles of
row 1, then of row sh-2; item 2 tiles + j is row 1 + j of columns 1 and sw-2.  A wave looks at 64 items per round and 256 per trip
of its `base` loop."""
import numpy as np

import helpers as H
import ring_batch_scenes as B
import work_cut_scenes as S

LIGHT, DARK = 235, 20
MIN_FRAMES = 9                     # the ring kernels run in batches of more than 8 frames
MAX_CLEARED, MAX_REACH = 5, 3      # a dot's cleared ring pixels: how many at most, how far from the target at most


def bgr(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def plane_stride(sw):
    return (sw + 15) & ~15


def ring_items(sw, sh):
    """(tiles, items) of the ring of a sw x sh plane"""
    tiles = plane_stride(sw) >> 4
    return tiles, 2 * tiles + sh - 2


def column_item(sw, sh, y):
    """the item that holds ring row y of columns 1 and sw-2"""
    return 2 * ring_items(sw, sh)[0] + y - 1


def cleared(binary):
    """ring pixels [(x, y)] of a binary image (non-zero = set; the 1-px frame is not looked at) that are not set, in the order
    top row, bottom row, left column, right column"""
    b = np.asarray(binary) > 0
    sh, sw = b.shape
    out = [(int(x), 1) for x in np.flatnonzero(~b[1, 1:sw - 1]) + 1] + [(int(x), sh - 2) for x in np.flatnonzero(~b[sh - 2, 1:sw - 1]) + 1]
    for x in (1, sw - 2):
        out += [(x, int(y)) for y in np.flatnonzero(~b[2:sh - 2, x]) + 2]
    return out


def rule(binary):
    """the verdict ring_quads_kernel owes a binary image: 1 exactly when both sides are at least 8 and the ring is all set"""
    sh, sw = np.asarray(binary).shape
    return int(sw >= 8 and sh >= 8 and not cleared(binary))


def dot_reaches(holes, target):
    return (target in holes and len(holes) <= MAX_CLEARED
            and all(max(abs(x - target[0]), abs(y - target[1])) <= MAX_REACH for x, y in holes))


def find_dot(g, target, box=None, before=(), alone=False):
    """draws into grey frame g the first dot -- 1 x 1, then 2 x 2, on or touching the target -- after which the oracle's binary image
    of the ROI box = (x0, y0, w, h) of g (the whole frame by default) has lost ring pixel `target` (ROI coordinates) and what
    `before` lists, and nothing else, within the bounds above; returns (x, y, size) in frame coordinates, or None (g unchanged).
    alone: the target must be the only ring pixel lost, and dots of 3 x 3 and dots one pixel further away are tried as well --
    the binarise smooths over 2 x 2 blocks, and a pixel with an odd coordinate never goes alone with the smaller dots"""
    Hh, W = g.shape
    x0, y0, w, h = box or (0, 0, W, Hh)
    want_kept = set(before)
    for size in (1, 2, 3) if alone else (1, 2):
        # the dots that cover the target first, then those beside it
        offs = sorted(((dx, dy) for dy in range(-size - alone, 2 + alone) for dx in range(-size - alone, 2 + alone)),
                      key=lambda o: (not (o[0] <= 0 < o[0] + size and o[1] <= 0 < o[1] + size), abs(o[0]) + abs(o[1]), o))
        for dx, dy in offs:
            x, y = x0 + target[0] + dx, y0 + target[1] + dy
            if x < 0 or y < 0 or x + size > W or y + size > Hh or (g[y:y + size, x:x + size] != LIGHT).any():
                continue
            g[y:y + size, x:x + size] = DARK
            holes = [p for p in cleared(H.oracle_binarise(g[y0:y0 + h, x0:x0 + w])) if p not in want_kept]
            if holes == [target] if alone else dot_reaches(holes, target):
                return x, y, size
            g[y:y + size, x:x + size] = LIGHT
    return None


_cache = {}


def cached(fn):
    def get(*a):
        if (fn.__name__, a) not in _cache:
            _cache[(fn.__name__, a)] = fn(*a)
        return _cache[(fn.__name__, a)]
    return get


# ---- frame rings by position (ring_quads_kernel<false>) -------------------------------------------------------------------------
# size -> the dark squares of its frames.  98 x 67: (sw-2) & 15 == 0, one trip of the base loop (78 items); 320 x 240: (sw-2) & 15
# == 14, (sh-2) % 14 == 0, two trips (278 items); 96 x 520: the same residues, three trips (530 items)
FRAME_SIZES = {(98, 67): [(34, 18, 30)], (320, 240): [(60, 60, 30), (200, 120, 40)], (96, 520): [(30, 100, 30), (34, 300, 36)],
               (34, 18): []}
SEAM_ITEMS = (63, 64, 255, 256, 511, 512)   # the last item of a round or trip and the first of the next


def frame_targets(W, Hh):
    """name -> ring pixel of a W x Hh frame's plane: the corners; the tile seams, the second and the last tile's first and last ring
    column on the top and bottom rows; the tile-row seams, the second and the last but one ring row on both columns; the column
    items on either side of a 64-item and a 256-item seam"""
    sw, sh = W & ~1, Hh & ~1
    last0 = max(((sw - 2) >> 4) << 4, 1)
    t = {"corner_tl": (1, 1), "corner_tr": (sw - 2, 1), "corner_bl": (1, sh - 2), "corner_br": (sw - 2, sh - 2)}
    for row, y in (("top", 1), ("bottom", sh - 2)):
        for x in (2, 15, 16, 17, last0, sw - 2):
            if 1 < x <= sw - 2:
                t["%s_x%d" % (row, x)] = (x, y)
    ys = [2, 13, 14, 15, sh - 3] + [1 + i - 2 * ring_items(sw, sh)[0] for i in SEAM_ITEMS]
    for col, x in (("left", 1), ("right", sw - 2)):
        for y in ys:
            if 1 < y < sh - 2:
                t["%s_y%d" % (col, y)] = (x, y)
    # (98 x 67: the last tile's only ring column is the corner's; a name per pixel)
    seen, out = set(), {}
    for name, p in t.items():
        if p not in seen:
            out[name] = p
            seen.add(p)
    return out


def base_frame(W, Hh):
    g = np.full((Hh, W), LIGHT, np.uint8)
    for x, y, s in FRAME_SIZES[(W, Hh)]:
        g[y:y + s, x:x + s] = DARK
    return g


@cached
def frame_scene(W, Hh):
    """(grey frames [n, Hh, W], names [n], targets [n]) of one size: the clean frame, then one frame per target of frame_targets
    with the dot that opens the ring there.  A target no dot reaches raises"""
    targets = frame_targets(W, Hh)
    frames, names, where = [base_frame(W, Hh)], ["clean"], [None]
    for name, p in targets.items():
        g = base_frame(W, Hh)
        if find_dot(g, p) is None:
            raise AssertionError("no dot opens the ring of a %d x %d frame at %s %s" % (W, Hh, name, p))
        frames.append(g)
        names.append(name)
        where.append(p)
    # the highest column of a full tile's run and a tile row's last row, as the only pixel cleared: where a dot gives that
    sw, sh = W & ~1, Hh & ~1
    for name, p in (("top_x15_alone", (15, 1)), ("bottom_x15_alone", (15, sh - 2)), ("top_x31_alone", (31, 1)),
                    ("left_y13_alone", (1, 13)), ("right_y13_alone", (sw - 2, 13))):
        g = base_frame(W, Hh)
        if p[0] < sw - 2 and p[1] < sh - 2 and find_dot(g, p, alone=True) is not None:
            frames.append(g)
            names.append(name)
            where.append(p)
    return np.stack(frames), names, where


# ---- the frames' grid-stride loop: more than 4096 frames --------------------------------------------------------------------------
STRIDE_W, STRIDE_H, STRIDE_FRAMES = 34, 18, 4100


@cached
def stride_scene():
    """(distinct grey frames [k, 18, 34], index of every frame of the batch [4100]): frame 0 is clean; every third frame of the
    batch has a hole, cycling over the targets of the 34 x 18 plane"""
    frames, names, _ = frame_scene(STRIDE_W, STRIDE_H)
    n_holed = len(frames) - 1
    index = np.array([1 + (f // 3) % n_holed if f % 3 == 2 else 0 for f in range(STRIDE_FRAMES)])
    return frames, index


# ---- crop rings by shape and position (ring_quads_kernel<true>) -----------------------------------------------------------------
CW, CH, CROP_FRAMES = 320, 300, 10
# dark rectangles (x, y, w, h) every frame holds: the four parities of a crop's sides, two more shapes, one whose crop has more
# than 256 ring items, and more of the first kinds to fill the batch
CROP_RECTS = [(100, 40, 30, 30), (150, 40, 31, 30), (200, 40, 30, 31), (250, 40, 31, 31), (100, 95, 37, 29), (160, 95, 33, 60),
              (50, 25, 30, 250), (215, 95, 30, 30), (100, 150, 31, 31), (215, 150, 31, 30), (100, 205, 30, 31), (160, 180, 37, 29),
              (215, 205, 30, 30)]
EDGE_OFFSETS = (3, 4, 5)


def edge_rect(side, off):
    """a dark rectangle `off` px from one frame edge"""
    return {"left": (off, 130, 24, 30), "top": (120, off, 30, 24), "right": (CW - off - 24, 130, 24, 30),
            "bottom": (130, CH - off - 24, 30, 24)}[side]


def clipped(side, roi):
    _, x0, y0, w, h = roi
    return {"left": x0 == 0, "top": y0 == 0, "right": x0 + w == CW, "bottom": y0 + h == CH}[side]


def draw_rects(rects):
    g = np.full((CH, CW), LIGHT, np.uint8)
    for x, y, w, h in rects:
        g[y:y + h, x:x + w] = DARK
    return g


def oracle_crops(g):
    """the crop ROIs [(owner, x0, y0, w, h)] the oracle's frame pass gives grey frame g"""
    return S.crop_rois(H.oracle_find_squares(g), g.shape[1], g.shape[0])


@cached
def edge_rects():
    """side -> the rectangle nearest its edge (3 .. 5 px) of which the oracle keeps a quad whose crop that edge clips, or None"""
    out = {}
    for side in ("left", "top", "right", "bottom"):
        out[side] = None
        for off in EDGE_OFFSETS:
            r = edge_rect(side, off)
            if any(clipped(side, c) for c in oracle_crops(draw_rects([r]))):
                out[side] = r
                break
    return out


def crop_hole_kinds(sw, sh):
    """name -> ring pixel of a sw x sh crop plane"""
    return {"corner_tl": (1, 1), "corner_tr": (sw - 2, 1), "corner_bl": (1, sh - 2), "corner_br": (sw - 2, sh - 2),
            "top_x15": (15, 1), "top_x16": (16, 1), "top_x17": (17, 1), "bottom_x15": (15, sh - 2), "bottom_x16": (16, sh - 2),
            "bottom_x17": (17, sh - 2), "top_last": (sw - 3, 1), "bottom_last": (sw - 3, sh - 2),
            "left_y13": (1, 13), "left_y14": (1, 14), "left_y15": (1, 15), "right_y13": (sw - 2, 13), "right_y14": (sw - 2, 14),
            "right_y15": (sw - 2, 15), "right_mid": (sw - 2, sh // 2), "left_end": (1, sh - 4), "right_end": (sw - 2, sh - 4),
            "top_x15_alone": (15, 1), "left_y13_alone": (1, 13)}


KIND_NAMES = list(crop_hole_kinds(40, 40))
# what the crop of more than 256 items gets, frame by frame: its rows sh-4 are column items of the second trip
TALL_KINDS = [None, "left_end", "right_end", "corner_br", None, "right_mid", "left_y14", "bottom_x16", "right_end", "left_end"]


@cached
def crop_scene():
    """(grey frames [10, 300, 320], plan): every frame holds every rectangle; plan[f] = [(roi, kind or None, target or None)] is
    what the generator did to the crops of frame f, as the oracle gives them for the frame without dots.  Every other crop of the
    batch (counted through its frames) is left as it is; the others get the next kind of hole in turn, or none where no dot gives
    it (a crop that lies inside its dark rectangle)"""
    rects = CROP_RECTS + [r for r in edge_rects().values() if r is not None]
    base = draw_rects(rects)
    rois = oracle_crops(base)
    frames, plan, turn = [], [], 0
    for f in range(CROP_FRAMES):
        g = base.copy()
        rows = []
        for j, roi in enumerate(rois):
            _, x0, y0, w, h = roi
            sw, sh = w & ~1, h & ~1
            tall = ring_items(sw, sh)[1] > 256
            kind = TALL_KINDS[f % len(TALL_KINDS)] if tall else KIND_NAMES[turn % len(KIND_NAMES)] if (f * len(rois) + j) & 1 else None
            target = None
            if kind is not None:
                target = crop_hole_kinds(sw, sh)[kind]
                before = cleared(H.oracle_binarise(g[y0:y0 + h, x0:x0 + w]))
                if find_dot(g, target, (x0, y0, w, h), before, alone=kind.endswith("_alone")) is None:
                    kind = target = None
                elif not tall:
                    turn += 1
            rows.append((roi, kind, target))
        frames.append(g)
        plan.append(rows)
    return np.stack(frames), plan


def crop_rings(g):
    """the crops of grey frame g as the oracle gives them, [(x0, y0, w, h, cleared ring pixels)]"""
    return [(x0, y0, w, h, cleared(H.oracle_binarise(g[y0:y0 + h, x0:x0 + w]))) for _, x0, y0, w, h in oracle_crops(g)]


# ---- the crops' grid-stride loop: more ROIs than 9 frames x 32 waves x 64 --------------------------------------------------------
DENSE_W, DENSE_H, DENSE_FRAMES, DENSE_SIDE, DENSE_PITCH = 1920, 1080, 9, 24, 30
DENSE_QUADS, DENSE_MARKERS = 4096, 64   # the context's limits per frame
DENSE_MIN_ROIS = DENSE_FRAMES * 32 * 64


@cached
def dense_scene():
    """(distinct grey frames [2, 1080, 1920], index of every frame of the batch [9]): dark squares of 24 on a pitch of 30; every
    fifth square -- counted from 0 in the first frame, from 2 in the second -- has a dot in the gap to its left, the one find_dot
    finds for the left column of one square's crop"""
    slots = [(x, y) for y in range(8, DENSE_H - DENSE_SIDE - 8, DENSE_PITCH) for x in range(8, DENSE_W - DENSE_SIDE - 8, DENSE_PITCH)]
    g = np.full((DENSE_H, DENSE_W), LIGHT, np.uint8)
    for x, y in slots:
        g[y:y + DENSE_SIDE, x:x + DENSE_SIDE] = DARK
    # a 150 x 150 corner of the frame is enough to find the dot on: the crop of the square at slot (2, 2) of the grid
    part = np.ascontiguousarray(g[:150, :150])
    px, py = 8 + 2 * DENSE_PITCH, 8 + 2 * DENSE_PITCH
    roi = [c for c in oracle_crops(part) if c[1] < px < c[1] + c[3] and c[2] < py < c[2] + c[4]]
    assert len(roi) == 1, roi
    _, x0, y0, w, h = roi[0]
    dot = find_dot(part, (1, py + DENSE_SIDE // 2 - y0), (x0, y0, w, h))
    assert dot is not None, "no dot opens the ring of a dense scene's crop"
    dx, dy, size = dot[0] - px, dot[1] - py, dot[2]
    frames = []
    for first in (0, 2):
        f = g.copy()
        for k, (x, y) in enumerate(slots):
            if k % 5 == first:
                f[y + dy:y + dy + size, x + dx:x + dx + size] = DARK
        frames.append(f)
    return np.stack(frames), np.array([0, 1, 0, 0, 1, 0, 0, 1, 0])


# ---- stale flags ---------------------------------------------------------------------------------------------------------------
def stale_sequence():
    """the three batches (BGR frames) run in this order on one context: 130 crops in 9 frames; the same cut to 8 frames, which
    runs no ring kernel; 9 frames with one crop"""
    big = B.batch_of(130)[0]
    return [big, big[:8], B.batch_of(1)[0]]

"""Scenes and case tables for tests/test_gpu_work_cuts.py and tests/test_work_cuts_cpu.py: every way a batch is cut into work
units -- the crop binarise kernel's strips, units, row plans and grey panels; the frame kernel's chunk seams; the batch plan's
thresholds.  The scenes are drawn here in numpy; which crops they give is read from the oracle's quads (crop_rois restates
decode_core.h::crop_rect), and crop_classes names the classes of binarise.hip::march_unit<SRC_CROP, true> a list of crops
reaches.  The CPU test asserts the classes on the oracle's crops, the GPU test on the crops it reads back."""
import numpy as np

import helpers as H

MARCH_STRIP, MARCH_CROP_ROWS, PANEL = 240, 252, 240   # kernels.h: MARCH_STRIP, MARCH_CROP_ROWS; hd.h: GRAY_PANEL_COLS
QUIET = 3                                             # quiet zone of a drawn marker: the crop reaches 5 px past its square


def textured(w, h, seed):
    """grey background that stays busy after the binarise's blur: a diagonal ramp plus seeded 2 x 2 blocks of +-40"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    ramp = 128 + (24 * (xs * h + ys * w - w * h)) // (w * h)
    blocks = np.kron(rng.integers(-40, 41, ((h + 1) // 2, (w + 1) // 2)), np.ones((2, 2), np.int64))[:h, :w]
    return np.clip(ramp + blocks, 0, 255).astype(np.uint8)


def draw_marker(img, x, y, side, name="2x2-01", quiet=QUIET, side_y=None):
    """an upright marker (template cells sampled at the nearest cell, 20 / 235) with its top-left pixel at (x, y), side x side_y
    pixels, inside a light quiet zone; whatever lies outside img is cut off"""
    tpl = H.template_pixels()[name][0]
    n_y, n_x = tpl.shape
    side_y = side if side_y is None else side_y
    h, w = img.shape
    x0, x1, y0, y1 = max(x - quiet, 0), min(x + side + quiet, w), max(y - quiet, 0), min(y + side_y + quiet, h)
    if x0 >= x1 or y0 >= y1:
        return
    u, v = np.arange(x0, x1) - x, np.arange(y0, y1) - y
    cell = tpl[np.clip(v * n_y // side_y, 0, n_y - 1)[:, None], np.clip(u * n_x // side, 0, n_x - 1)[None, :]]
    inside = ((v >= 0) & (v < side_y))[:, None] & ((u >= 0) & (u < side))[None, :]
    img[y0:y1, x0:x1] = np.where(inside, np.where(cell > 0, 235, 20), 235).astype(np.uint8)


def frame_of(w, h, seed, markers):
    """BGR frame w x h: textured background, markers = [(x, y, side) or (x, y, side, side_y)]"""
    g = textured(w, h, seed)
    for m in markers:
        draw_marker(g, m[0], m[1], m[2], side_y=m[3] if len(m) > 3 else None)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def crop_rois(quads, W, H_):
    """decode_core.h::crop_rect and order.hip::setup_crop on the ordered frame-pass quads [n, 4, 2] of one W x H frame: the list
    of (owner, x0, y0, w, h) of the squares whose crop has a plane (even sides of at least 2)"""
    out = []
    for i, q in enumerate(np.asarray(quads, np.int64).reshape(-1, 4, 2)):
        rx, ry = max(int(q[:, 0].min()) - 5, 0), max(int(q[:, 1].min()) - 5, 0)
        rx1, ry1 = min(int(q[:, 0].max()) + 5, W), min(int(q[:, 1].max()) + 5, H_)
        w, h = rx1 - rx, ry1 - ry
        if (w & ~1) >= 2 and (h & ~1) >= 2:
            out.append((i, rx, ry, w, h))
    return out


def crop_classes(rois_by_frame, W, H_):
    """names of the classes the crops [(owner, x0, y0, w, h)] of the frames of one W x H batch reach"""
    got = set()
    for rois in rois_by_frame:
        if len(rois) >= 90:
            got.add("pool>=90")
        for _, x0, y0, w, h in rois:
            sw, sh = w & ~1, h & ~1
            for r in range(2, 16, 2):
                if sh == MARCH_CROP_ROWS + r:
                    got.add("last_unit_%d" % r)
            if sh > 2 * MARCH_CROP_ROWS:
                got.add("sh>504")
            if sh <= MARCH_CROP_ROWS:
                got.add("one_unit")
            for c in (2, 4):
                if sw == MARCH_STRIP + c:
                    got.add("last_strip_%d" % c)
            if MARCH_STRIP + 16 <= sw <= 2 * MARCH_STRIP:
                got.add("last_strip>=16")
            if sw > 2 * MARCH_STRIP:
                got.add("sw>480")
            if sw < 32:
                got.add("sw<32")       # the byte-load path (plan = sw >= 32 is false)
            if sw in (32, 34):
                got.add("sw=32|34")    # the first sizes of the one-load row plan
            if sh < 32:
                got.add("sh<32")
            got.add("x0&3=%d" % (x0 & 3))
            if 232 <= x0 <= 240:
                got.add("x0=%d" % x0)
            if x0 < PANEL and x0 + w > 2 * PANEL:
                got.add("two_panel_boundaries")
            if x0 == 239 and sw > MARCH_STRIP:
                got.add("x0=239_wide")
            if W & 1 and x0 + w == W:
                got.add("odd_right_w%s" % ("even" if w % 2 == 0 else "odd"))
                if W - 1 == PANEL:
                    got.add("odd_right_begins_panel")
            if H_ & 1 and y0 + h == H_:
                got.add("odd_bottom_h%s" % ("even" if h % 2 == 0 else "odd"))
    return got


# ---- B: the crop scenes.  name -> (W, H, [frames' marker lists], the classes the scene is there for) -------------------------
def _seam_scene():
    # sides 226 .. 262: the outer square's crop (side + 10 or so) and the inner squares' sweep sw over 242, 244 and sh over 254 .. 266
    return 300, 300, [[(14 + k % 4, 16 + k % 3, 226 + k)] for k in range(37)], \
        {"last_unit_%d" % r for r in range(2, 16, 2)} | {"last_strip_2", "last_strip_4", "last_strip>=16", "one_unit"}


def _panel_scene():
    frames = [[(30, 30, 500)]]                                   # three strips, three units, two panel boundaries
    for k in range(4):                                           # small markers whose crops begin at 230 .. 243, three per frame
        frames.append([(243 + k, 8, 262)] + [(235 + 3 * j + k + (12 if j == 3 else 0), 290 + 66 * j, 52) for j in range(4)])
    return 560, 560, frames, {"sh>504", "sw>480", "two_panel_boundaries", "x0=239_wide", "x0=240"} | {"x0=%d" % x for x in range(232, 240)} \
        | {"x0&3=%d" % k for k in range(4)}


BAR_THICKNESS = tuple(range(2, 26, 2))


def _edge_scene():
    # 241 x 241: column 240 begins a grey panel and is the odd last column; row 240 is the odd last row.  Markers against and
    # across the right edge, the bottom edge and the corner; slivers of a 120-px marker 8 .. 30 px wide
    frames = []
    for k in range(6):
        frames.append([(241 - 64 - k, 20 + k, 60), (20 + k, 241 - 64 - k, 60), (120, 120, 60 + 55 + k)])
    for vis in range(8, 32, 2):
        frames.append([(241 - vis, 10, 120), (10, 241 - vis - 1, 120), (-120 + vis + 1, 110, 120)])
    for vis in (14, 20, 26, 30, 34, 40):                          # a marker cut by the corner to vis x vis and a bit
        frames.append([(241 - vis, 241 - vis - 1, 160), (-160 + vis, -160 + vis + 2, 160)])
    # bars of 150 px, BAR_THICKNESS thick, lying and standing: the square finder keeps a quad of more than 500 px^2, so the
    # thinnest bars give no crop and the next ones the shortest and narrowest crops there are (the last frames of the scene)
    for t in BAR_THICKNESS:
        frames.append([(30, 40, 150, t), (200 - (t & 2), 30, t, 150)])
    return 241, 241, frames, {"sw<32", "sh<32", "sw=32|34", "odd_right_weven", "odd_right_wodd", "odd_right_begins_panel",
                              "odd_bottom_heven", "odd_bottom_hodd"}


def _pool_scene():
    # one frame of 10 x 10 markers of 30 px, in a batch of 9 (the two-phase crop pass and ring_quads run from 9 frames on)
    dense = [(8 + 43 * i + (j & 3), 8 + 43 * j + (i & 1), 30) for j in range(10) for i in range(10)]
    frames = [dense] + [[(20 + 7 * k, 30 + 5 * k, 90 + 6 * k), (250, 240 + 3 * k, 60 + 4 * k)] for k in range(8)]
    return 440, 440, frames, {"pool>=90"}


CROP_SCENES = {"seams": _seam_scene, "panels": _panel_scene, "edges": _edge_scene, "pool": _pool_scene}
# every class of the issue's list; each must be reached by some scene
CROP_CLASSES = ({"last_unit_%d" % r for r in range(2, 16, 2)} | {"sh>504", "one_unit", "last_strip_2", "last_strip_4", "last_strip>=16", "sw>480",
                "sw<32", "sw=32|34", "sh<32", "two_panel_boundaries", "x0=239_wide", "x0=240", "pool>=90",
                "odd_right_weven", "odd_right_wodd", "odd_right_begins_panel", "odd_bottom_heven", "odd_bottom_hodd"}
                | {"x0=%d" % x for x in range(232, 240)} | {"x0&3=%d" % k for k in range(4)})

_scene_cache = {}


def crop_scene(name):
    """(W, H, frames [n, H, W, 3], wanted classes) of a crop scene, drawn once"""
    if name not in _scene_cache:
        W, H_, lists, want = CROP_SCENES[name]()
        seed0 = sorted(CROP_SCENES).index(name) * 1000
        _scene_cache[name] = (W, H_, np.stack([frame_of(W, H_, seed0 + k, m) for k, m in enumerate(lists)]), want)
    return _scene_cache[name]


# ---- C: the frame kernel's chunk seams.  (width, height, min_units or None, formats, the classes the case is there for) ------
ALL_FORMATS = ("bgr", "rgb", "bgra", "rgba", "gray")
TWO_FORMATS = ("bgr", "gray")
CHUNK_CASES = [
    (64, 1262, None, ALL_FORMATS, {"last_2", "rows%4=0", "one_strip", "chunks>=3"}),
    (64, 1263, None, TWO_FORMATS, {"last_2", "odd_height"}),
    (64, 1264, None, TWO_FORMATS, {"last_4"}),
    (64, 1266, None, TWO_FORMATS, {"last_6"}),
    (64, 1268, None, TWO_FORMATS, {"last_8"}),
    (64, 1270, None, TWO_FORMATS, {"last_10"}),
    (64, 1272, None, TWO_FORMATS, {"last_12"}),
    (64, 1274, None, TWO_FORMATS, {"last_14"}),
    (242, 1262, None, TWO_FORMATS, {"last_2", "second_strip_2"}),
    (244, 378, None, TWO_FORMATS, {"second_strip_4", "rows%4=2", "last>=16"}),
    (64, 1388, None, TWO_FORMATS, {"fewer_chunks_than_planned"}),
    (64, 1262, 5, TWO_FORMATS, {"halved_once", "chunks>=3"}),
    (64, 1262, 2, TWO_FORMATS, {"halved_twice", "chunks=2"}),
    (64, 1262, 1, TWO_FORMATS, {"chunks=1"}),
]
CHUNK_CLASSES = ({"last_%d" % r for r in range(2, 16, 2)} | {"last>=16", "rows%4=0", "rows%4=2", "chunks=1", "chunks=2", "chunks>=3", "halved_once",
                 "halved_twice", "fewer_chunks_than_planned", "one_strip", "second_strip_2", "second_strip_4", "odd_height"})


def chunk_classes(width, height, min_units, default_plan, this_plan):
    """classes of a chunk case from its plan under the default min_units (default_plan) and under its own (this_plan): objects
    with frame_strips, frame_chunks, frame_chunk_rows, sw, sh (plan_emul's output)"""
    p, got = this_plan, set()
    last = p.sh - (p.frame_chunks - 1) * p.frame_chunk_rows
    got.add("last_%d" % last if last < 16 else "last>=16")
    got.add("rows%%4=%d" % (p.frame_chunk_rows % 4))
    got.add("chunks=%d" % p.frame_chunks if p.frame_chunks < 3 else "chunks>=3")
    began = max(1, (p.sh + 64) // 128)   # plan_core.h: the chunk count the plan begins with
    if min_units is None and p.frame_chunks < began:
        got.add("fewer_chunks_than_planned")
    if min_units is not None and 1 < p.frame_chunks < default_plan.frame_chunks:
        got.add("halved_once" if p.frame_chunks * 2 >= default_plan.frame_chunks else "halved_twice")
    if p.frame_strips == 1:
        got.add("one_strip")
    if p.frame_strips == 2 and p.sw - MARCH_STRIP in (2, 4):
        got.add("second_strip_%d" % (p.sw - MARCH_STRIP))
    if height & 1:
        got.add("odd_height")
    return got


def seam_rows(plan):
    """first rows of chunks 1 .. of a plan: the rows a seam marker is drawn across"""
    return [k * plan.frame_chunk_rows for k in range(1, plan.frame_chunks)]


def chunk_frames(width, height, seams, seed):
    """the two frames of a chunk case, BGR: seeded noise, and a textured frame with a marker drawn across every seam row (as many
    as fit; a frame narrower than a marker gets the widest that fits)"""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (height, width, 3), np.uint8)
    side = min(48, width - 12)
    rows = sorted(set(seams)) or [height // 2]
    # (a marker across a seam in the frame's last rows is cut by the frame's bottom edge)
    marks = [((6 + 5 * k) % max(1, width - side - 8) + 4, max(r - side // 2 - (k % 3), 4), side) for k, r in enumerate(rows)]
    return np.stack([noise, frame_of(width, height, seed + 1, marks)])


# ---- D: one scene of 8 distinct 320 x 240 frames -----------------------------------------------------------------------------
def plan_scene():
    """(frames [8, 240, 320, 3], poison [8, 240, 320, 3]): six textured marker frames, one sawtooth frame whose borders outlive
    tiers 1 and 2, one noise frame; and eight other frames of the same size to run through a context before every run"""
    from border_shapes import sawtooth_frame
    if "plan" not in _scene_cache:
        rng = np.random.default_rng(77)
        fr = [frame_of(320, 240, 500 + k, [(12 + 9 * k, 10 + 4 * k, 70 + 6 * k), (170 + 5 * k, 120 - 6 * k, 56 + 3 * k), (190 - 8 * k, 20 + k, 40 + 2 * k)])
              for k in range(6)]
        # (borders of 600 .. 1300 steps: past tier 1's 96; past tier 2's budget where that is 128 -- up to 8 frames -- or set lower)
        fr.append(sawtooth_frame(320, 240, 4, [(12, 12, 308, 132), (20, 148, 140, 228), (170, 150, 300, 226)]))
        fr.append(rng.integers(0, 256, (240, 320, 3), np.uint8))
        poison = [frame_of(320, 240, 900 + k, [(200 - 20 * k, 30 + 10 * k, 64 + 5 * k), (20 + 11 * k, 130 - 9 * k, 80)]) for k in range(7)]
        poison.append(rng.integers(0, 256, (240, 320, 3), np.uint8))
        _scene_cache["plan"] = (np.stack(fr), np.stack(poison))
    return _scene_cache["plan"]

"""Markers whose code grid is not square (width != height), for tests/test_nonsquare_cpu.py and tests/test_gpu_nonsquare.py.

A template of w x h cells is the rectangle (+-w/h, +-1) of the plane z = 0 (the object points of cvarSquareInit at
ratio = w/h), placed at a pose (R, t), projected through a CvarCamera (the pinhole camera of helpers.oracle_camera, or the DIST
lens of tests/persp_synth.py) and drawn with ocvar_synth_draw_quads over a white quiet zone on a light background.  Seeded and
deterministic; nothing is read from a file.

Library A holds the templates that are planted, library B sixteen extreme shapes that are never planted: under it every
square of the same frames is read through patches of 64x1 ... 1x63 cells.

pose_is_defined() says whether the reference itself defines the pose of a record: a square nobody matched is reported as a
score-0 record of template 0, and with a non-square template 0 (4x2 here) its rectangle is fitted to a quad of another shape.
On fronto-parallel views that fit has two nearly equal minima, and one float32 ulp of a corner coordinate decides between
them, in the reference as much as in this library."""
import ctypes as C
import math

import numpy as np

import board_chain as BC
import helpers as H
import persp_synth as PS
from helpers import P

WIDTH, HEIGHT = 640, 480
BACKGROUND = 200
QUIET = 0.4            # the quiet zone's margin around the rectangle, in units of its short half side
TILTS = (25, 45, 60)
SHORT_PX, LONG_PX = 60, 210   # the short side is SHORT_PX wide, unless the long side would pass LONG_PX (16x4, 4x16)
N_TILTED, N_FRONTAL = 16, 4
LIBRARY_SEED = 46      # a draw in which some template holds a light block of cells enclosed by dark ones: the oracle finds that
                       # block as a square of its own, and read through library B it sets every bit, the sign bit included
SEEDS = {"tilted": 20, "frontal": 21}
# Which in-plane quadrant of a template the oracle decodes depends on the corner its square finder starts at.  The seed of each
# tilted frame was searched (on the oracle alone) so that the frame's markers of quadrants 0 and 1 decode under both cameras
# (frame 1 has no such seed among the first 400: its templates decode in frame 13).
FRAME_SEEDS = [5, 0, 1, 22, 6, 58, 10, 26, 373, 7, 79, 9, 0, 5, 1, 25]
POSE_RTOL = 1e-4       # the project's pose bar
STABLE_RTOL = POSE_RTOL / 10   # what the reference may spend of it on one ulp of its input

# (width, height) in cells; the index is the template id
SIZES_A = [(4, 2), (2, 4), (8, 4), (4, 8), (3, 5), (5, 3), (6, 8), (8, 6), (7, 2), (2, 7), (6, 4), (4, 6), (16, 4), (4, 16),
           (9, 7), (7, 9)]
SIZES_B = [(64, 1), (1, 64), (32, 2), (2, 32), (21, 3), (3, 21), (16, 4), (4, 16), (13, 4), (4, 13), (12, 5), (5, 12), (10, 6),
           (6, 10), (63, 1), (1, 63)]
SIZES = {"A": SIZES_A, "B": SIZES_B}

_libraries = {}


def _grid(rng, w, h):
    """random cells with the corners fixed: no code of the grid is 0 or all ones"""
    g = rng.integers(0, 2, (h, w))
    g[0, 0], g[-1, -1] = 1, 0
    if w > 1 and h > 1:
        g[0, -1], g[-1, 0] = 0, 1
    return g


def library(which):
    """(names, CvarTemplate array, grids) of library 'A' or 'B'; the grids are registered with helpers under their names.
    No code of a template of library A equals a code of another of its templates"""
    if which not in _libraries:
        rng = np.random.default_rng([LIBRARY_SEED, ord(which)])
        while True:
            grids = [_grid(rng, w, h) for w, h in SIZES[which]]
            names = ["ns%s-%dx%d" % (which, w, h) for w, h in SIZES[which]]
            for n, g in zip(names, grids):
                H.register_template(n, g)
            tpls = H.oracle_templates(names)
            # (code[1..3] come out of acBitRotate, whose index formulas are a square grid's: with w != h the cells it would read
            # outside the grid are 0, in the oracle as in the host library)
            codes = [set(int(c) for c in t.code) for t in tpls]
            if which == "B" or all(codes[i].isdisjoint(codes[j]) for i in range(len(codes)) for j in range(i)):
                break   # (library B is never planted: its codes only have to be read)
        assert [(t.width, t.height) for t in tpls] == SIZES[which]
        _libraries[which] = (names, tpls, grids)
    return _libraries[which]


def camera(lens=False):
    return PS.camera(WIDTH, HEIGHT, lens)


def rectangle(ratio, margin=0.0):
    m = margin * min(ratio, 1.0)
    return np.array([[-ratio - m, -1 - m], [ratio + m, -1 - m], [ratio + m, 1 + m], [-ratio - m, 1 + m]], np.float64)


def pose(cam, u, v, short_px, ratio, tilt_deg, gamma_deg, phi_deg):
    """(R, t): the rectangle's centre projects (pinhole) to pixel (u, v), its short side is about short_px wide there, it is
    rotated in plane by gamma and tilted by tilt about the in-plane axis at angle phi"""
    K, _ = BC.cam_arrays(cam)
    g, ph = math.radians(gamma_deg), math.radians(phi_deg)
    Rz = np.array([[math.cos(g), -math.sin(g), 0], [math.sin(g), math.cos(g), 0], [0, 0, 1]])
    R = BC.rodrigues(np.array([math.cos(ph), math.sin(ph), 0]) * math.radians(tilt_deg)) @ Rz
    Z = K[0, 0] * 2.0 * min(ratio, 1.0) / short_px
    return R, np.array([(u - K[0, 2]) / K[0, 0] * Z, (v - K[1, 2]) / K[1, 1] * Z, Z])


def project(cam, R, t, ratio, margin=0.0):
    K, dist = BC.cam_arrays(cam)
    return BC.project(K, dist, R, t, rectangle(ratio, margin))


def short_side(w, h):
    r = max(w, h) / min(w, h)
    return min(SHORT_PX, LONG_PX / r)


def _disjoint(a, b):
    """two convex quads [4, 2] do not meet (a separating axis among their edge normals)"""
    for poly in (a, b):
        e = np.roll(poly, -1, axis=0) - poly
        for n in np.c_[-e[:, 1], e[:, 0]]:
            pa, pb = a @ n, b @ n
            if pa.max() < pb.min() or pb.max() < pa.min():
                return True
    return False


def _fits(cams, planted, ratios):
    """under every camera: the quiet zones lie inside the frame and no marker touches another marker's quiet zone"""
    for cam in cams:
        quiet = [project(cam, R, t, r, QUIET) for (R, t), r in zip(planted, ratios)]
        inner = [project(cam, R, t, r) for (R, t), r in zip(planted, ratios)]
        for q in quiet:
            if q[:, 0].min() < 3 or q[:, 1].min() < 3 or q[:, 0].max() > WIDTH - 4 or q[:, 1].max() > HEIGHT - 4:
                return False
        for i in range(len(planted)):
            for j in range(len(planted)):
                if i != j and not _disjoint(inner[i], quiet[j]):
                    return False
    return True


def frame_plan(f):
    """[(template, quadrant, tilt)] of the four cells of tilted frame f: over the 16 frames every template of library A
    appears once in each in-plane quadrant, and sees every tilt"""
    out = []
    for c in range(4):
        tpl = (f + 4 * c) % 16
        q = (f // 4 + 2 * c) % 4
        out.append((tpl, q, TILTS[(tpl + q) % 3]))
    return out


_poses = {}


def poses(family):
    """family 'tilted': 16 lists of four (template, quadrant, tilt, R, t), one marker near the centre of each cell of a 2 x 2
    grid; 'frontal': 4 lists with the templates of the first four tilted frames at tilt 0, one marker of each centred on the
    principal point and the others placed where they fit.  The poses fit the frame under both cameras"""
    if family in _poses:
        return _poses[family]
    rng = np.random.default_rng(SEEDS[family])
    cams = [camera(False), camera(True)]
    K, _ = BC.cam_arrays(cams[0])
    out = []
    for f in range(N_TILTED if family == "tilted" else N_FRONTAL):
        plan = frame_plan(f)
        ratios = [SIZES_A[tpl][0] / SIZES_A[tpl][1] for tpl, _, _ in plan]
        if family == "tilted":
            rng = np.random.default_rng([SEEDS[family], f, FRAME_SEEDS[f]])
        for attempt in range(4000):
            planted = []
            for c, (tpl, q, tilt) in enumerate(plan):
                gamma = 90 * q + rng.uniform(-20, 20)
                if family == "tilted":
                    u = (c % 2 + 0.5 + rng.uniform(-0.08, 0.08)) * WIDTH / 2
                    v = (c // 2 + 0.5 + rng.uniform(-0.08, 0.08)) * HEIGHT / 2
                elif c == f % 4:
                    u, v, tilt = K[0, 2], K[1, 2], 0
                else:
                    u, v, tilt = rng.uniform(40, WIDTH - 40), rng.uniform(40, HEIGHT - 40), 0
                planted.append(pose(cams[0], u, v, short_side(*SIZES_A[tpl]), ratios[c], tilt, gamma, rng.uniform(0, 360)))
            if _fits(cams if family == "tilted" else cams[:1], planted, ratios):
                break
        else:
            raise AssertionError(("no placement", family, f))
        out.append([(tpl, q, 0 if family == "frontal" else tilt, R, t) for (tpl, q, tilt), (R, t) in zip(plan, planted)])
    _poses[family] = out
    return out


def render(cam, planted):
    """planted: [(template, quadrant, tilt, R, t)] -> (bgr frame, [PS.PlantedMarker]); every quiet zone is drawn first"""
    names, _, _ = library("A")
    tp = H.template_pixels()
    arrs = [np.ascontiguousarray(tp[n][0]) for n in names] + [np.full((4, 4), 255, np.uint8)]
    st = (H.SynthTemplate * len(arrs))()
    for i, a in enumerate(arrs):
        st[i].pixels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        st[i].h, st[i].w = a.shape
    ratios = [SIZES_A[p[0]][0] / SIZES_A[p[0]][1] for p in planted]
    quads = ([project(cam, p[3], p[4], r, QUIET) for p, r in zip(planted, ratios)] +
             [project(cam, p[3], p[4], r) for p, r in zip(planted, ratios)])
    tidx = np.ascontiguousarray([len(names)] * len(planted) + [p[0] for p in planted], np.int32)
    q = np.ascontiguousarray((np.array(quads) + 0.5).reshape(-1, 8))   # (the generator's pixel (x, y) covers [x, x + 1))
    bgr = np.full((HEIGHT, WIDTH, 3), BACKGROUND, np.uint8)
    n = BC.synth().ocvar_synth_draw_quads(P(bgr), WIDTH, HEIGHT, WIDTH * 3, st, len(arrs), P(tidx), P(q), len(tidx))
    assert n == len(tidx)
    markers = [PS.PlantedMarker(quads[len(planted) + i], p[3], p[4], p[0], p[2], short_side(*SIZES_A[p[0]]), tag=p[1])
               for i, p in enumerate(planted)]
    return bgr, markers


_scenes = {}


def scenes(family):
    """'pinhole' / 'lens': the 16 tilted frames through that camera; 'frontal': the 4 frontal frames (pinhole)"""
    if family not in _scenes:
        cam = camera(family == "lens")
        out = []
        for f, planted in enumerate(poses("frontal" if family == "frontal" else "tilted")):
            frame, markers = render(cam, planted)
            out.append(PS.Scene(family, "%s-%d" % (family, f), frame, markers, cam, family == "lens"))
        _scenes[family] = out
    return _scenes[family]


FAMILIES = ("pinhole", "lens", "frontal")


# ---- the reference's own stability ---------------------------------------------------------------------------------------

def pose_movement(square, ratio, cam):
    """the most the oracle's glMatrix of a square moves, relative to max(1, |g|max), when one of the eight coordinates goes to
    the next float32 up or down (nan if a pose is not finite)"""
    o = H.oracle()
    sq = np.ascontiguousarray(np.asarray(square, np.float32).reshape(8))
    g0 = np.zeros(16)
    o.orc_square_to_matrix(P(sq), C.byref(cam), C.c_double(ratio), P(g0))
    scale = max(1.0, np.abs(g0).max())
    worst = 0.0
    for i in range(8):
        for to in (np.float32(np.inf), np.float32(-np.inf)):
            s = sq.copy()
            s[i] = np.nextafter(sq[i], to)
            g = np.zeros(16)
            o.orc_square_to_matrix(P(s), C.byref(cam), C.c_double(ratio), P(g))
            d = np.abs(g - g0).max() / scale
            if d != d:
                return float("nan")
            worst = max(worst, d)
    return float(worst)


def pose_is_defined(square, ratio, cam):
    """the reference's pose of this square is stable: none of the 16 one-ulp moves of a corner coordinate moves its glMatrix
    by more than POSE_RTOL / 10"""
    return pose_movement(square, ratio, cam) <= STABLE_RTOL


# ---- the oracle on the frames, once per process -----------------------------------------------------------------------------

class Run:
    """the oracle on one scene under one library: records, candidates, grey image, and per record the movement of its pose"""

    def __init__(self, scene, tpls, prev=None):
        self.scene = scene
        self.ref, self.cands, img = H.oracle_registration(scene.frame, tpls, scene.cam, prev=prev, max_cands=48 * len(tpls))
        self.gray = np.ascontiguousarray(img[:, :, 0])
        self.movement = [pose_movement(np.array(r.square, np.float32), r.aspectRatio, scene.cam) for r in self.ref]
        self.defined = [m <= STABLE_RTOL for m in self.movement]


_runs = {}


def runs(which, family):
    """[Run] of the family's scenes under library 'A' or 'B'"""
    key = (which, family)
    if key not in _runs:
        tpls = library(which)[1]
        _runs[key] = [Run(s, tpls) for s in scenes(family)]
    return _runs[key]


def crop_of(gray, quad):
    """the crop cvarArMultRegistration decodes a frame quad in: its bounding box and 5 px, clipped by the frame"""
    h, w = gray.shape
    x0, y0 = max(quad[:, 0].min() - 5, 0), max(quad[:, 1].min() - 5, 0)
    x1, y1 = min(quad[:, 0].max() + 5, w), min(quad[:, 1].max() + 5, h)
    return gray[y0:y1, x0:x1], int(x1 - x0), int(y1 - y0)


# ---- template files ------------------------------------------------------------------------------------------------------------

def write_png(path, pixels):
    """an 8-bit grey PNG of a template image (the 1-cell black frame included), one pixel per cell"""
    import struct
    import zlib

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    px = np.asarray(pixels, np.uint8)
    h, w = px.shape
    raw = b"".join(b"\0" + px[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def templates_from_png(host, directory):
    """library A written as PNG files into directory and loaded with cvarLoadTemplateTag of the host library: [helpers.Template]"""
    import os
    names, _, _ = library("A")
    tp = H.template_pixels()
    host.cvarLoadTemplateTag.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    out = []
    for n in names:
        path = os.path.join(str(directory), n + ".png")
        write_png(path, tp[n][0])
        t = H.Template()
        assert host.cvarLoadTemplateTag(C.byref(t), path.encode(), 0.01) == 1, n
        out.append(t)
    return out

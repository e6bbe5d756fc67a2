"""Camera views of single markers for tests/test_perspective_cpu.py and tests/test_gpu_perspective.py: every marker is the square
(-1,-1) (1,-1) (1,1) (-1,1) of the plane z = 0 (the object points of cvarSquareInit at ratio 1) placed in space at a known pose
(R, t), projected through a CvarCamera -- pinhole, or the five-coefficient model with the DIST lens -- and drawn with
ocvar_synth_draw_quads over a light quiet zone on a light background.  Seeded and deterministic; nothing is read from a file.

A frame holds at most one marker of each template: cvarArMultRegistration's dedupe keeps one candidate per template."""
import ctypes as C
import math

import numpy as np

import board_chain as BC
import helpers as H
from helpers import P

DIST = [-0.21, 0.09, 0.0015, -0.0008, -0.02]   # the lens of tests/test_device_cores_cpu.py (k1 k2 p1 p2 k3)
NAMES = H.TEMPLATE_ORDER + H.BIG_TEMPLATES     # 2x2 ... 8x8; template id = index
TILTS = (0, 30, 50, 60, 70, 75)
OBJ = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)
QUIET = 1.4          # the quiet zone is the marker's square scaled by this about its centre
BACKGROUND = 200
WHITE = len(NAMES)   # index of the all-white "template" that draws the quiet zones


class PlantedMarker:
    """quad: the true image corners [4, 2] of the outer edge (pixel centres at integers), corner c the projection of OBJ[c]"""

    def __init__(self, quad, R, t, template, tilt, size, tag=None):
        self.quad, self.R, self.t, self.template, self.tilt, self.size, self.tag = quad, R, t, template, tilt, size, tag


class Scene:
    def __init__(self, family, name, frame, markers, cam, lens):
        self.family, self.name, self.frame, self.markers, self.cam, self.lens = family, name, frame, markers, cam, lens
        self.height, self.width = frame.shape[:2]


def camera(width, height, lens=False, wide=1.0):
    """the default camera scaled to the frame; wide > 1 shortens the focal lengths (a wide-angle view)"""
    cam = H.oracle_camera(width, height)
    cam.cameraMatrix[0] /= wide
    cam.cameraMatrix[4] /= wide
    if lens:
        cam.distCoeffs[:] = DIST
    return cam


def pose(cam, u, v, size_px, tilt_deg, gamma_deg, phi_deg):
    """(R, t): the marker's centre projects (pinhole) to pixel (u, v), its side is about size_px wide there, it is rotated in
    plane by gamma and tilted by tilt about the in-plane axis at angle phi"""
    K, _ = BC.cam_arrays(cam)
    g, ph = math.radians(gamma_deg), math.radians(phi_deg)
    Rz = np.array([[math.cos(g), -math.sin(g), 0], [math.sin(g), math.cos(g), 0], [0, 0, 1]])
    R = BC.rodrigues(np.array([math.cos(ph), math.sin(ph), 0]) * math.radians(tilt_deg)) @ Rz
    Z = K[0, 0] * 2.0 / size_px
    return R, np.array([(u - K[0, 2]) / K[0, 0] * Z, (v - K[1, 2]) / K[1, 1] * Z, Z])


def project(cam, R, t, scale=1.0):
    K, dist = BC.cam_arrays(cam)
    return BC.project(K, dist, R, t, OBJ * scale)


def _templates():
    tp = H.template_pixels()
    arrs = [np.ascontiguousarray(tp[n][0]) for n in NAMES] + [np.full((4, 4), 255, np.uint8)]
    st = (H.SynthTemplate * len(arrs))()
    for i, a in enumerate(arrs):
        st[i].pixels = a.ctypes.data_as(C.POINTER(C.c_uint8))
        st[i].h, st[i].w = a.shape
    return arrs, st


def render(width, height, cam, planted):
    """planted: [(R, t, template, tilt, size, tag)] -> (bgr frame, [PlantedMarker]); every quiet zone is drawn before any marker"""
    arrs, st = _templates()
    bgr = np.full((height, width, 3), BACKGROUND, np.uint8)
    quads = [project(cam, R, t, QUIET) for R, t, *_ in planted] + [project(cam, R, t) for R, t, *_ in planted]
    tidx = np.ascontiguousarray([WHITE] * len(planted) + [p[2] for p in planted], np.int32)
    q = np.ascontiguousarray((np.array(quads) + 0.5).reshape(-1, 8))   # (the generator's pixel (x, y) covers [x, x + 1))
    BC.synth().ocvar_synth_draw_quads(P(bgr), width, height, width * 3, st, len(arrs), P(tidx), P(q), len(tidx))
    return bgr, [PlantedMarker(quads[len(planted) + i], *p) for i, p in enumerate(planted)]


def scene(family, name, width, height, specs, lens=False, wide=1.0):
    """specs: [(u, v, size_px, tilt, gamma, phi, template, tag)]"""
    cam = camera(width, height, lens, wide)
    planted = [pose(cam, u, v, s, tilt, g, ph) + (tpl, tilt, s, tag) for u, v, s, tilt, g, ph, tpl, tag in specs]
    frame, markers = render(width, height, cam, planted)
    return Scene(family, name, frame, markers, cam, lens)


ANY_ROTATION = (0, 2, 6, 7, 8)   # 2x2, 4x4, 8x8: the other widths decode in one rotation only (the stride quirk of the code reader)


def gamma_of(rng, template, quadrant):
    """an in-plane angle in the given quadrant, or in the first one for a template that decodes only there"""
    return 90 * (quadrant % 4 if template in ANY_ROTATION else 0) + 45 + rng.uniform(-25, 25)


def grid_specs(rng, width, height, cols, rows, size_of, tilt_of, first_quadrant=0):
    """one marker per cell of a cols x rows grid, cell c with template c, near the cell's centre"""
    out = []
    for c in range(cols * rows):
        u = (c % cols + 0.5 + rng.uniform(-0.08, 0.08)) * width / cols
        v = (c // cols + 0.5 + rng.uniform(-0.08, 0.08)) * height / rows
        out.append((u, v, size_of(c), tilt_of(c), gamma_of(rng, c % len(NAMES), c + first_quadrant), rng.uniform(0, 360),
                    c % len(NAMES), None))
    return out


LADDER_SIZES = (160, 140, 120, 100, 80, 60, 45, 32)
LADDER_REPEATS = 6


def ladder(lens=False, seed=101, sizes=LADDER_SIZES):
    """the tilt ladder: 960x540 frames with four markers of one apparent width each.  The six frames of a width hold every
    tilt four times; templates and in-plane quadrants rotate through the cells from frame to frame (the four of a frame differ)"""
    rng = np.random.default_rng(seed)
    family = "lens" if lens else "ladder"
    out = []
    for s, size in enumerate(LADDER_SIZES):
        for r in range(LADDER_REPEATS):
            specs = []
            for c in range(4):
                u = (c % 2 + 0.5 + rng.uniform(-0.08, 0.08)) * 480
                v = (c // 2 + 0.5 + rng.uniform(-0.08, 0.08)) * 270
                tpl = (13 * s + 4 * r + c) % len(NAMES)   # (13: the tilt of a cell must not fix its template)
                specs.append((u, v, size, TILTS[(4 * r + c) % 6], gamma_of(rng, tpl, c + r + s), rng.uniform(0, 360), tpl, None))
            if size in sizes:   # (the random stream does not depend on the selection)
                out.append(scene(family, "%s-%d-%d" % (family, size, r), 960, 540, specs, lens))
    return out


EDGE_DISTANCES = (0, 1, 2, 5, 6)


def _at_distance(cam, width, height, size, tilt, gamma, phi, side_x, side_y, d):
    """the image centre (u, v) that puts the outer quad's drawn extent d px from the frame's edges named by side_x, side_y
    (-1: left / top, +1: right / bottom, 0: centred on that axis)"""
    u, v = width / 2.0, height / 2.0
    for _ in range(8):
        q = project(cam, *pose(cam, u, v, size, tilt, gamma, phi)) + 0.5
        if side_x:
            u += (d - q[:, 0].min()) if side_x < 0 else (width - d - q[:, 0].max())
        if side_y:
            v += (d - q[:, 1].min()) if side_y < 0 else (height - d - q[:, 1].max())
    return u, v


EDGE_PLACES = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]


def edges(seed=202):
    """960x540 frames (the ladder's size: one batch holds both families), for each distance d one with four markers d px from the four edges and one with four markers d px from
    both edges of the four corners of the frame (d px of background between the frame's edge and the nearest drawn marker
    pixel), and two frames of markers that the frame's edge cuts"""
    rng = np.random.default_rng(seed)
    W, Hh = 960, 540
    out = []
    for i, d in enumerate(EDGE_DISTANCES + (-12,)):
        cam = camera(W, Hh)
        for half in (0, 1):
            specs = []
            for k, (sx, sy) in enumerate(EDGE_PLACES[4 * half:4 * half + 4]):
                tpl = (8 * i + 4 * half + k) % len(NAMES)
                size, tilt, gamma, phi = 64 + 8 * k, (30, 0, 50, 60)[(k + i) % 4], gamma_of(rng, tpl, k + i), rng.uniform(0, 360)
                u, v = _at_distance(cam, W, Hh, size, tilt, gamma, phi, sx, sy, d)
                specs.append((u, v, size, tilt, gamma, phi, tpl, (d, sx, sy)))
            name = ("edges-d%d" % d if d >= 0 else "edges-cut") + ("-corners" if half else "-sides")
            out.append(scene("edges", name, W, Hh, specs))
    return out


PANEL_WIDTHS = (231, 249, 471, 489)


def sizes(seed=303):
    """frame sizes: 1920x1080 and 1921x1081 (nine markers, mixed tilts), widths 240 k +- 9 with a marker corner on the grey
    plane's panel boundary column (240, 480) or, below 240, next to the last column, 64x48, 32x48 (narrower than the 33 px of
    the refinement's widest patch, and the smallest such frame in which the oracle finds a marker), the 17x33 and 40x18 frames of test_smallest_frames_and_markers_cut_by_the_frame_edge
    (a marker there is below the area cut: nothing may be reported), and one 3840x2160 frame"""
    rng = np.random.default_rng(seed)
    out = []
    for (w, h) in ((1920, 1080), (1921, 1081)):
        specs = grid_specs(rng, w, h, 3, 3, lambda c: 150 - 12 * c, lambda c: TILTS[c % 5])
        out.append(scene("sizes", "sizes-%dx%d" % (w, h), w, h, specs))
    for w in PANEL_WIDTHS:
        h = w * 3 // 4
        cam = camera(w, h)
        specs = []
        cols = [c for c in (240, 480) if c < w] or [w - 9]
        for k, col in enumerate(cols):
            size, tilt, gamma, phi = 70, 30, 25.0 + 25 * k, 40.0
            u, v = w / 2.0, h * (0.5 if len(cols) == 1 else 0.27 + 0.46 * k)
            for _ in range(16):   # the corner nearest the column lands on it
                q = project(cam, *pose(cam, u, v, size, tilt, gamma, phi))
                j = int(np.argmax(q[:, 0])) if col >= w - 10 else int(np.argmin(np.abs(q[:, 0] - col)))
                u += col - q[j, 0]
            specs.append((u, v, size, tilt, gamma, phi, k, ("column", col)))
        out.append(scene("sizes", "sizes-w%d" % w, w, h, specs))
    out.append(scene("sizes", "sizes-64x48", 64, 48, [(31.5, 23.5, 34, 0, 10.0, 0.0, 0, None)]))
    out.append(scene("sizes", "sizes-32x48", 32, 48, [(15.5, 23.5, 20, 0, 0.0, 0.0, 0, None)]))
    out.append(scene("sizes", "sizes-17x33", 17, 33, [(8.0, 16.0, 11, 0, 0.0, 0.0, 0, None)]))
    out.append(scene("sizes", "sizes-40x18", 40, 18, [(19.5, 8.5, 12, 0, 0.0, 0.0, 0, None)]))
    specs = grid_specs(rng, 3840, 2160, 3, 3, lambda c: 300 - 30 * c, lambda c: TILTS[(c + 2) % 6])
    out.append(scene("sizes", "sizes-3840x2160", 3840, 2160, specs))
    return out


def off_axis(seed=404):
    """a wide-angle camera (focal lengths divided by 2.5) with untilted and tilted markers in the corners of a 1280x720 image"""
    rng = np.random.default_rng(seed)
    out = []
    for f, tilt in enumerate((0, 50)):
        specs = []
        for k, (sx, sy) in enumerate(EDGE_PLACES):
            u = 640 + sx * 520 + rng.uniform(-10, 10)
            v = 360 + sy * 260 + rng.uniform(-10, 10)
            tpl = (k + 3 * f) % len(NAMES)
            specs.append((u, v, 90 + 6 * k, tilt, gamma_of(rng, tpl, k), rng.uniform(0, 360), tpl, None))
        out.append(scene("off-axis", "off-axis-tilt%d" % tilt, 1280, 720, specs, wide=2.5))
    return out


def lens():
    """the tilt ladder's poses (same seed) through the distorted camera, at four of its widths"""
    return ladder(lens=True, sizes=(160, 120, 80, 45))


_all = None


def all_scenes():
    global _all
    if _all is None:
        _all = ladder() + edges() + sizes() + off_axis() + lens()
    return _all


def steepest():
    """the ladder frames of the two largest widths (every tilt, twice each, at the sizes where the steep ones are found)"""
    return [s for s in all_scenes() if s.family == "ladder"][:2 * LADDER_REPEATS]


# ---- records against the ground truth -------------------------------------------------------------------------------------

def pose_of_glmatrix(gl):
    """(R, t) of cvarGlMatrix's 16 doubles: it stores diag(-1,-1,1) R^T diag(-1,-1,1) row by row and (tx, ty, -tz)"""
    m = np.asarray(gl, np.float64).reshape(4, 4)
    D = np.diag([-1.0, -1.0, 1.0])
    return (D @ m[:3, :3] @ D).T, np.array([m[3, 0], m[3, 1], -m[3, 2]])


def _inside(p, quad):
    e = np.roll(quad, -1, axis=0) - quad
    c = e[:, 0] * (p[1] - quad[:, 1]) - e[:, 1] * (p[0] - quad[:, 0])
    return (c > 0).all() or (c < 0).all()


def match(square, planted, max_px=6.0):
    """(marker, k, d) of a record's square: the planted marker whose quad holds the square's centre (None if there is none); if
    the square is that marker's outer edge -- every corner within max_px of the truth under the best cyclic shift, record
    corner (c + k) & 3 at truth corner c -- that k, else (an inner border, a clipped quad) k = None"""
    s = np.asarray(square, np.float64).reshape(4, 2)
    for m in planted:
        if _inside(s.mean(axis=0), m.quad):
            k, d = BC.truth_shift(s, m.quad)
            return (m, k, d) if d <= max_px else (m, None, d)
    return None, None, np.inf


def truth_errors(gl, marker, k):
    """(rotation error in degrees, translation error relative to the distance) of a record's glMatrix against the planted
    pose: the record's corner j is object point OBJ[j], so with record corner (c + k) & 3 on truth corner c the record's
    rotation is the planted one turned by -90 k degrees in the marker's plane"""
    R, t = pose_of_glmatrix(gl)
    a = -math.pi / 2 * k
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    return BC.rt_errors(R, t, marker.R @ Rz, marker.t)


def tilt_bin(tilt):
    return min(TILTS, key=lambda b: abs(b - tilt))

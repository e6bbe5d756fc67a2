"""Camera views (tests/persp_synth.py: tilt up to 75 degrees, markers at the frame's edge, small frames, a wide-angle and a
distorting camera) on the CPU: what the oracle finds in them, the oracle's poses against the poses the markers were rendered
from, and the host builds of the device's decode and pose cores (tests/emul) against the oracle on every candidate.

The constants below were measured from the oracle on these scenes (never from the device path); the tests print what they
measure next to them (pytest -s)."""
import collections
import ctypes as C

import numpy as np
import pytest

import board_chain as BC
import helpers as H
import persp_synth as PS
import refine_chain as RC
from helpers import P

SET5 = (5, 30, 0.1)
LARGE = 100   # px: the apparent width from which a marker counts as large in the error table

# markers the oracle reports on a planted marker's outer edge, per tilt of the ladder (every bin must hold at least 8)
LADDER_COUNTS = {0: 29, 30: 23, 50: 24, 60: 21, 70: 10, 75: 13}
# records the oracle reports per family (records on inner borders and clipped quads included)
FAMILY_COUNTS = {"ladder": 122, "edges": 17, "sizes": 25, "off-axis": 9, "lens": 63}
# records on markers d px from the frame's edge (at 0 px the outer border touches the zeroed frame: an inner border is reported)
EDGE_COUNTS = {0: 1, 1: 2, 2: 4, 5: 4, 6: 6}

# The oracle's worst rotation error (degrees) and translation error (relative to the distance) against the planted pose, per
# tilt and size class, over all families: (unrefined, refined with half window 5).  The bound of a bin is twice its worst.
# Unrefined corners are integer vertices.  Where a worst is tens of degrees the oracle ended in the mirror minimum of the
# planar fit (reprojection cost of those poses: 0.002 .. 0.8 px^2, the device core's pose equal to 1e-14): that happens to
# markers below 100 px only.
TRUTH_WORST = {
    # (tilt, large): ((rot, trans) unrefined, (rot, trans) refined)
    (0, False): ((44.75, 0.0215), (4.05, 0.0325)),   # n = 29
    (0, True): ((6.83, 0.0056), (0.98, 0.0025)),   # n = 29
    (30, False): ((79.33, 0.0151), (5.42, 0.0288)),   # n = 31
    (30, True): ((2.15, 0.0049), (0.84, 0.0052)),   # n = 19
    (50, False): ((4.22, 0.0247), (126.39, 0.0198)),   # n = 21
    (50, True): ((1.25, 0.0183), (0.83, 0.0132)),   # n = 23
    (60, False): ((76.47, 0.0289), (4.30, 0.0235)),   # n = 18
    (60, True): ((1.25, 0.0062), (0.46, 0.0097)),   # n = 23
    (70, False): ((95.92, 0.0084), (2.19, 0.0181)),   # n = 9
    (70, True): ((1.58, 0.0170), (0.36, 0.0096)),   # n = 11
    (75, False): ((2.37, 0.0103), (1.01, 0.0162)),   # n = 5
    (75, True): ((1.29, 0.0186), (1.46, 0.0172)),   # n = 14
}


@pytest.fixture(scope="module")
def Lr():
    return RC.build_emul()


@pytest.fixture(scope="module")
def tpls():
    return H.oracle_templates(PS.NAMES)


class Run:
    """the oracle on one scene: records, candidates, grey image, frame quads, records refined by the host chain"""

    def __init__(self, scene, tpls, Lr):
        self.scene = scene
        self.ref, self.cands, img = H.oracle_registration(scene.frame, tpls, scene.cam)
        self.gray = np.ascontiguousarray(img[:, :, 0])
        self.refined = RC.refined_markers(Lr, self.ref, self.gray, scene.cam, SET5)
        self.matches = [PS.match(np.array(r.square), scene.markers) for r in self.ref]


@pytest.fixture(scope="module")
def runs(tpls, Lr):
    return [Run(s, tpls, Lr) for s in PS.all_scenes()]


def test_glmatrix_inverse_is_cvarGlMatrix_inverted():
    o = H.oracle()
    o.orc_gl_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(1)
    for _ in range(200):
        R = BC.rodrigues(rng.normal(size=3) * rng.uniform(0, 1.9))
        t = rng.normal(size=3) * 10
        gl = np.zeros(16)
        o.orc_gl_matrix(P(np.ascontiguousarray(R.reshape(-1))), P(t), P(gl))
        R2, t2 = PS.pose_of_glmatrix(gl)
        assert np.abs(R2 - R).max() < 1e-9 and np.abs(t2 - t).max() == 0


def test_scenes_are_deterministic_and_cover_the_families():
    sc = PS.all_scenes()
    assert {s.family for s in sc} == {"ladder", "edges", "sizes", "off-axis", "lens"}
    assert {(s.width, s.height) for s in sc} >= {(1920, 1080), (1921, 1081), (64, 48), (32, 48), (17, 33), (40, 18), (3840, 2160)} | {
        (w, w * 3 // 4) for w in PS.PANEL_WIDTHS}
    again = PS.ladder()[:2] + PS.edges()[:2]
    first = [s for s in sc if s.family == "ladder"][:2] + [s for s in sc if s.family == "edges"][:2]
    assert all(np.array_equal(a.frame, b.frame) for a, b in zip(again, first))
    lad = [m for s in sc if s.family == "ladder" for m in s.markers]
    assert {m.tilt for m in lad} == set(PS.TILTS) and {m.template for m in lad} == set(range(len(PS.NAMES)))
    # a planted corner lies on the grey plane's panel boundary column (or, below 240, within 9 columns of the last one)
    for s in sc:
        if s.name.startswith("sizes-w"):
            for m in s.markers:
                col = m.tag[1]
                assert np.abs(m.quad[:, 0] - col).min() < 1e-3 and (col % 240 == 0 or s.width - col <= 9)
    # the edge family's markers are where their tags say (drawn extent: the quad + 0.5)
    for s in sc:
        for m in s.markers:
            if s.family == "edges" and m.tag[0] >= 0:
                d, sx, sy = m.tag
                q = m.quad + 0.5
                if sx:
                    assert abs((q[:, 0].min() if sx < 0 else s.width - q[:, 0].max()) - d) < 1e-3
                if sy:
                    assert abs((q[:, 1].min() if sy < 0 else s.height - q[:, 1].max()) - d) < 1e-3


def census(runs):
    ladder, family, edge = collections.Counter(), collections.Counter(), collections.Counter()
    for r in runs:
        family[r.scene.family] += len(r.ref)
        for m, k, d in r.matches:
            if r.scene.family == "ladder" and k is not None:
                ladder[m.tilt] += 1
            if r.scene.family == "edges" and m is not None:
                edge[m.tag[0]] += 1
    return dict(ladder), dict(family), dict(edge)


def test_what_the_oracle_finds(runs):
    ladder, family, edge = census(runs)
    print("\noracle markers per ladder tilt: %s\nrecords per family: %s\nrecords per edge distance: %s" % (
        sorted(ladder.items()), sorted(family.items()), sorted(edge.items())))
    assert ladder == LADDER_COUNTS and family == FAMILY_COUNTS
    assert {d: n for d, n in edge.items() if d >= 0} == EDGE_COUNTS
    assert all(ladder[t] >= 8 for t in PS.TILTS)
    assert all(edge.get(d, 0) >= 1 for d in PS.EDGE_DISTANCES)
    for r in runs:   # a marker the frame's edge cuts, or one below the area cut, is not reported
        if r.scene.name.startswith("edges-cut") or r.scene.name in ("sizes-17x33", "sizes-40x18"):
            assert len(r.ref) == 0 and len(r.cands) == 0, r.scene.name
        if r.scene.name in ("sizes-64x48", "sizes-32x48") or r.scene.name.startswith("sizes-w"):
            assert sum(k is not None for _, k, _ in r.matches) >= 1, r.scene.name
    # all four starting corners occur among the records, and decodes in all four orientations
    assert {k for r in runs for _, k, _ in r.matches if k is not None} == {0, 1, 2, 3}
    assert {c.orient for r in runs for c in r.cands} == {0, 1, 2, 3, 4}


def truth_table(runs, records_of):
    """(tilt, large) -> [worst rotation error, worst translation error, n] over the records on outer edges"""
    worst = {}
    for r in runs:
        for rec, (m, k, d) in zip(records_of(r), r.matches):
            if k is None:
                continue
            ang, rel = PS.truth_errors(np.array(rec.glMatrix), m, k)
            w = worst.setdefault((m.tilt, m.size >= LARGE), [0.0, 0.0, 0])
            w[0], w[1], w[2] = max(w[0], ang), max(w[1], rel), w[2] + 1
    return worst


def check_truth(table, column, what):
    print("\n%s against the planted poses: (tilt, large) -> worst rotation (deg), worst translation / distance, n" % what)
    for key in sorted(table):
        print("    %s: %.2f  %.4f  %d   (recorded worst %s)" % (key, *table[key], TRUTH_WORST[key][column]))
    assert set(table) == set(TRUTH_WORST)
    for key, (ang, rel, n) in table.items():
        w_ang, w_rel = TRUTH_WORST[key][column]
        assert ang <= 2 * w_ang and rel <= 2 * w_rel, (what, key, ang, rel)


@pytest.mark.parametrize("refine", [False, True])
def test_oracle_poses_against_the_planted_poses(runs, refine):
    """the single-marker corner order and glMatrix convention against something other than the oracle: a swapped axis or a
    corner order off by one costs 90 degrees or more; the large bins' bounds are below 14 degrees"""
    table = truth_table(runs, (lambda r: r.refined) if refine else (lambda r: r.ref))
    check_truth(table, int(refine), "oracle, refined" if refine else "oracle")
    assert max(w[int(refine)][0] for k, w in TRUTH_WORST.items() if k[1]) < 7.0


def crop_of(gray, quad):
    """the crop cvarArMultRegistration decodes a frame quad in: its bounding box and 5 px, clipped by the frame"""
    h, w = gray.shape
    x0, y0 = max(quad[:, 0].min() - 5, 0), max(quad[:, 1].min() - 5, 0)
    x1, y1 = min(quad[:, 0].max() + 5, w), min(quad[:, 1].max() + 5, h)
    return gray[y0:y1, x0:x1], int(x1 - x0), int(y1 - y0)


def reprojection_cost(gl, square, cam):
    R, t = PS.pose_of_glmatrix(gl)
    return float(np.sum((PS.project(cam, R, t) - np.asarray(square, np.float64).reshape(4, 2)) ** 2))


def test_device_cores_against_the_oracle(emul, runs, tpls):
    """emul_read_code on every oracle candidate (bit-exact) and emul_square_to_glmatrix on every candidate square and every
    refined record square, pinhole and lens, at the host-to-host bar of test_decode_and_pose_cores.  The device's Cholesky LM
    and the oracle's pseudo-inverse LM do not part on these scenes (measured: 1.8e-9 at most); were they to, the device's
    reprojection cost must not be the higher one."""
    o = H.oracle()
    emul.emul_square_to_glmatrix.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    n_codes = n_poses = clipped = decoded = 0
    worst = 0.0
    for r in runs:
        s = r.scene
        quads = H.oracle_find_squares(r.gray)
        squares = {}
        for c in r.cands:
            crop, cw, ch = crop_of(r.gray, quads[c.markerId])
            clipped += cw < np.ptp(quads[c.markerId][:, 0]) + 10 or ch < np.ptp(quads[c.markerId][:, 1]) + 10
            t = tpls[c.templateId]
            pp = np.array(c.patPoint, np.float32)
            bit = emul.emul_read_code(C.c_void_p(crop.ctypes.data), cw, ch, s.width, P(pp), t.width, t.height)
            assert bit == c.bit, (s.name, c.markerId, c.templateId)
            n_codes += 1
            decoded += c.orient > 0
            squares[bytes(c.square)] = (np.array(c.square, np.float32), 1.0)
        for m in r.refined:
            squares[bytes(m.square)] = (np.array(m.square, np.float32), m.aspectRatio)
        for sq, ratio in squares.values():
            g1, g2 = np.zeros(16), np.zeros(16)
            o.orc_square_to_matrix(P(sq), C.byref(s.cam), C.c_double(ratio), P(g1))
            emul.emul_square_to_glmatrix(P(sq), C.byref(s.cam), C.c_double(ratio), P(g2))
            rel = np.abs(g1 - g2).max() / max(1.0, np.abs(g1).max())
            worst = max(worst, rel)
            if ratio == 1.0:
                c1, c2 = reprojection_cost(g1, sq, s.cam), reprojection_cost(g2, sq, s.cam)
                assert c2 <= c1 * (1 + 1e-6) + 1e-9, (s.name, sq.tolist(), c1, c2)   # (both stop at a relative step of FLT_EPSILON)
            assert rel <= 1e-6, (s.name, sq.tolist(), rel)
            n_poses += 1
    print("\ndevice cores: %d codes (%d decoded, %d in crops the frame clips), %d poses, worst pose difference %.2g" % (
        n_codes, decoded, clipped, n_poses, worst))
    assert n_codes >= 2000 and decoded >= 200 and clipped >= 20 and n_poses >= 400

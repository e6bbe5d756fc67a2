"""Frames whose quad-owning borders sit at the follower's slab, pool and key-width limits (follow.hip, kernels.h), shared by
tests/test_follow_limits_cpu.py -- which proves on the oracle that every scene reaches the classes it names -- and
tests/test_gpu_follow_limits.py, which runs them on the GPU.

A border *owns* a quad of oracle_find_squares when all four vertices are points of it; of several such borders the one with
the most points.  Only owning borders count here: the points of a border that yields no quad never reach a result.

Classes a scene can name (Scene.classes), each about one owning border:
  n=<N>            it has exactly N corner points (then N % 64 is the last store of tier 3's lane-parked points)
  key32 / key64    which keys wave_approx_dp's maximum searches take: 32-bit when n <= 1024 and the squared diagonal of the
                   bounding box is < 2^21, else 64-bit; key64:box -- n <= 1024, the box alone decides; key64:n -- the box is
                   well inside, the count alone decides; diag2=<D> pins the squared diagonal
  vertex@64, vertex@1024, vertex@8192
                   a quad vertex, as orc_approx_poly picks it on the oracle's contour, is the last point before or the first
                   point after a seam: a non-zero multiple of 64 (tier 3's stores, the staging loops), index 1024 (the lane
                   slab's end, LDS_PTS, the 32-bit keys' count), index 8192 (the wave slab's end)

Tier 2 (follow.hip::follow_mid_kernel) parks a walk's points during a block of MID_BLOCK = 32 *steps* and then flushes however
many points those steps produced, so its flush seams are no multiples of anything: they are the point counts at every 32nd
step of the border's own walk, which tier2_marks takes from the host build of tier 2.  Classes from them (tier2_classes), for a
border of at most SLAB_PTS points -- tier 2 finishes it from the slab it flushed to:
  t2last=<K>       the flush after the walk's last block holds K points (0: the walk closes without a point left to flush)
  t2full           at least one block whose 32 steps all yield a point: a full LDS row, every lane of the flush group stores
  vertex@t2flush   a quad vertex is the last point of one flush or the first of the next
and for a border of more points, which follow_overflow follows again, so that the slab's contents reach no result:
  t2cut=<K>/<P>    of the P points of the block that crosses SLAB_PTS only K are flushed; the points after them stay parked in
                   the LDS row -- from the 32nd such point on (borders of 1056 points and more) in its spare slot
"""
from collections import namedtuple

import numpy as np

import helpers as H
from border_shapes import sawtooth_frame
from helpers import P

SLAB_PTS = 1024         # kernels.h; LDS_PTS in follow.hip is the same number, and so is the 32-bit keys' count limit
SLAB3_PTS = 8192        # kernels.h
MID_BLOCK = 32          # follow.hip
KEY32_DIAG2 = 1 << 21   # follow.hip::wave_finish_packed
SEAMS = {"vertex@64": 64, "vertex@1024": SLAB_PTS, "vertex@8192": SLAB3_PTS}

Scene = namedtuple("Scene", "name w h make classes seam_only")
Owner = namedtuple("Owner", "quad contour n hole start bbox diag2 vertex_index")


def saw(w, h, x1, y1, x0=40, y0=40):
    return lambda: sawtooth_frame(w, h, 2, [(x0, y0, x1, y1)])


def square(w, h, side, x0=60, y0=30):
    def make():
        img = np.full((h, w, 3), 220, np.uint8)
        img[y0:y0 + side, x0:x0 + side] = 20
        return img
    return make


def rhombus(w, h, a, b):
    """a dark rhombus |x - w/2| / a + |y - h/2| / b <= 1: with a = 2 b its border turns at every step"""
    def make():
        y, x = np.mgrid[0:h, 0:w]
        img = np.full((h, w), 220, np.uint8)
        img[np.abs(x - w // 2) * b + np.abs(y - h // 2) * a <= a * b] = 20
        return np.repeat(img[:, :, None], 3, axis=2)
    return make


def _n(n):
    return ("n=%d" % n, "n%%64=%d" % (n % 64))


# Scene.classes: one group per owning border of the frame -- every quad's owner is named, with its exact count.  The counts
# are the oracle's; tests/test_follow_limits_cpu.py derives them again.  seam_only: a duplicate of another scene's classes
# but for where a vertex lies (frame pass only on the GPU).
SCENES = [
    # --- 640x480: SLAB_PTS = LDS_PTS = the 32-bit keys' count limit = 1024, both sides.  Tier 2's last flush: 18, 16, 1, 14, 3
    # and 17 points; the 1025- and 1026-point borders cross the slab's end inside a block of 21 points.
    # The third vertex of the 1023-point border is point 512: the first after a 64-point seam; the third vertex of the 716-point
    # border, point 358, is the first point of one of tier 2's flushes.
    Scene("saw640_1023", 640, 480, saw(640, 480, 377, 402),
          (_n(1023) + ("key32", "vertex@64", "t2last=18"), _n(720) + ("key32", "t2last=1")), False),
    Scene("saw640_1024", 640, 480, saw(640, 480, 375, 403), (_n(1024) + ("key32", "t2last=16"), _n(714) + ("key32", "t2last=14")), False),
    Scene("saw640_1025", 640, 480, saw(640, 480, 380, 401),
          (_n(1025) + ("key64", "key64:n", "t2cut=20/21"), _n(718) + ("key32", "t2last=3")), False),
    Scene("saw640_1026", 640, 480, saw(640, 480, 378, 402),
          (_n(1026) + ("key64", "key64:n", "t2cut=19/21"), _n(716) + ("key32", "t2last=17", "vertex@t2flush")), False),
    # rhombi whose sides rise 1 in 2: the outer border turns at every step, so tier 2 flushes full rows of 32 points (20 and 26
    # of them).  The first vertex of the 798-point border, point 600, is the first point of a flush; the second vertex of the
    # 478-point border, point 238, the last of one, and that border's walk closes with nothing left to flush.
    Scene("rhombus_201", 640, 480, rhombus(640, 480, 201, 100),
          (_n(798) + ("key32", "t2full", "t2last=8", "vertex@t2flush"), _n(388) + ("key32", "t2last=15")), False),
    Scene("rhombus_250", 640, 480, rhombus(640, 480, 250, 125),
          (_n(990) + ("key32", "t2full", "t2last=12"), _n(478) + ("key32", "t2last=0", "vertex@t2flush")), False),
    # --- 1280x1100: key width at few points -- the box alone decides.  Bounding box 1023 x 1023, squared diagonal 2^21 - 4094:
    # the largest the 32-bit keys take; 1024 x 1024, exactly 2^21: the first for the 64-bit keys; 1041 x 1041: well beyond
    Scene("square_1022", 1280, 1100, square(1280, 1100, 1022), (_n(13) + ("key32", "t2last=0"), _n(16) + ("key32", "diag2=2093058", "t2last=0")), False),
    Scene("square_1023", 1280, 1100, square(1280, 1100, 1023), (_n(20) + ("key32",), _n(8) + ("key64:box", "diag2=2097152")), False),
    Scene("square_1040", 1280, 1100, square(1280, 1100, 1040), (_n(13) + ("key64:box",), _n(16) + ("key64:box", "diag2=2167362")), False),
    # ... and a quad vertex (the third: the teeth of the left and the bottom side come before it) either side of the seam at
    # point 1024, on borders that tier 3 finishes from its slab without staging
    Scene("saw1280_vertex_1023", 1280, 1100, saw(1280, 1100, 741, 715), (_n(2041) + ("key64", "vertex@1024"), _n(1396) + ("key64",)), False),
    Scene("saw1280_vertex_1024", 1280, 1100, saw(1280, 1100, 742, 715), (_n(2042) + ("key64", "vertex@1024"), _n(1394) + ("key64",)), True),
    # --- 3840x2160: SLAB3_PTS = 8192, one below, at, one above; last store of 63, 0 and 1 points
    Scene("saw3840_8191", 3840, 2160, saw(3840, 2160, 3437, 2119), (_n(8191) + ("key64",), _n(5496) + ("key64",)), False),
    Scene("saw3840_8192", 3840, 2160, saw(3840, 2160, 3438, 2119), (_n(8192) + ("key64",), _n(5494) + ("key64",)), False),
    Scene("saw3840_8193", 3840, 2160, saw(3840, 2160, 3441, 2118), (_n(8193) + ("key64",), _n(5500) + ("key64",)), False),
    # the third vertex is point 4096: the first of a 64-point store of tier 3
    Scene("saw3840_vertex_4096", 3840, 2160, saw(3840, 2160, 3436, 2119), (_n(8188) + ("key64", "vertex@64"), _n(5490) + ("key64",)), True),
]
# vertex@8192 is not reached.  A sawtoothed rectangle's border starts at its top-left corner, and its last vertex comes one side
# before the end, at point n - (points of the last side).  Rectangles (40, 40, x1, y1) with x1 in 3430 .. 3445 and y1 in 2118 ..
# 2121 were searched: 8180 .. 8203 points, last vertex at point 5643 .. 5659.  No other rectangle does better: the largest that
# 3840x2160 holds has 8734 points, so a vertex at 8191 or 8192 leaves the last side 542 points at the most, and the three sides
# before it -- one of them as short as the last -- would need a height beyond the frame for their 8191 points.
SEAMS_LEFT_OUT = ("vertex@8192",)


def parity_frames():
    """the frames of the point-rich borders in tests/test_gpu_parity.py (test_borders_with_thousands_of_points,
    test_capacity_overflow_is_loud_not_wrong, test_pathological_noise_frames_are_handled_exactly), built as those tests build
    them: no border of more than 1024 points owns a quad there"""
    rng = np.random.default_rng(12)
    return {
        "thousands_0": sawtooth_frame(1280, 960, 6, [(100, 100, 700, 500), (800, 150, 1200, 900), (150, 600, 650, 880)]),
        "thousands_1": sawtooth_frame(1280, 960, 4, [(60, 60, 1220, 900)]),
        "capacity": sawtooth_frame(3840, 2160, 4, [(40, 40, 3800, 2120)]),
        "noise": np.ascontiguousarray(np.kron(rng.integers(0, 2, (1080 // 4, 1920 // 4, 1), np.uint8) * 255, np.ones((4, 4, 3), np.uint8))),
    }


# the tooth-2 frame test_borders_with_thousands_of_points adds: both long borders own a quad
def thousands_tooth2():
    return sawtooth_frame(1280, 960, 2, [(60, 60, 1220, 900)])


def contours(binary):
    """H.oracle_contours with buffers sized for these frames (a border point per pixel at the most)"""
    b = np.ascontiguousarray(binary)
    h, w = b.shape
    maxp, maxc = b.size + 16, b.size // 2 + 16
    pts = np.zeros(2 * maxp, np.int32)
    offs = np.zeros(maxc + 1, np.int32)
    starts = np.zeros(maxc, np.int32)
    holes = np.zeros(maxc, np.int32)
    n = H.oracle().orc_find_contours(P(b), w, h, P(pts), maxp, P(offs), P(starts), P(holes), maxc)
    assert n >= 0
    return [pts[2 * offs[i]:2 * offs[i + 1]].reshape(-1, 2) for i in range(n)], starts[:n].copy(), holes[:n].copy()


def approx(pts, eps=None):
    """orc_approx_poly of a closed contour at 0.02 x its perimeter, as orc_find_squares calls it"""
    p = np.ascontiguousarray(pts, np.int32)
    n = len(p)
    if eps is None:
        eps = H.oracle().orc_arc_length_closed(P(p), n) * 0.02
    out = np.zeros((n + 1, 2), np.int32)
    m = H.oracle().orc_approx_poly(P(p), n, eps, P(out))
    return out[:m].copy()


Analysis = namedtuple("Analysis", "gray binary contours starts holes quads owners")


def analyse(frame_bgr, min_pts=4):
    """the oracle's planes, contours and quads of a frame, and for every quad the border that owns it (min_pts > 4: only the
    quads that a border of at least min_pts points owns)"""
    gray = np.ascontiguousarray(frame_bgr[..., 0])
    binary = H.oracle_binarise(gray)
    cs, starts, holes = contours(binary)
    quads = H.oracle_find_squares(gray)
    sw = binary.shape[1]
    owners = []
    packed = {ci: (c[:, 1].astype(np.int64) << 16) | c[:, 0] for ci, c in enumerate(cs) if len(c) >= min_pts} if len(quads) else {}
    for qi, q in enumerate(quads):
        key = (q[:, 1].astype(np.int64) << 16) | q[:, 0]
        best = -1
        for ci, pk in packed.items():
            if (best < 0 or len(pk) > len(packed[best])) and np.isin(key, pk).all():
                best = ci
        if best < 0 and min_pts > 4:
            continue
        assert best >= 0, ("a quad no border owns", qi, q.tolist())
        c = cs[best]
        bw, bh = int(c[:, 0].max() - c[:, 0].min()), int(c[:, 1].max() - c[:, 1].min())
        vi = tuple(tuple(int(i) for i in np.flatnonzero(packed[best] == k)) for k in key)
        owners.append(Owner(qi, best, len(c), int(holes[best]), (int(starts[best]) % sw, int(starts[best]) // sw), (bw, bh),
                            bw * bw + bh * bh, vi))
    return Analysis(gray, binary, cs, starts, holes, quads, owners)


def walk_rows(lib, binary):
    """fe_walks (tests/emul/follow_emul.cpp, the `lib` fixture of test_follow_tiers_cpu.py) of every plausible start of a binary
    image: rows of fe_row_ints() ints"""
    b = np.ascontiguousarray((np.asarray(binary) > 0).astype(np.uint8))
    sh, sw = b.shape
    cap = 1 << 17
    rows = np.zeros((cap, 24), np.int32)
    n = lib.fe_walks(P(b), sw, sh, 1, P(rows), cap)
    assert 0 <= n <= cap
    return rows[:n]


def owner_row(rows, o, sw):
    """the row of owning border o: its start is the oracle's, at the bit plane's pitch"""
    ns = (sw + 15) & ~15
    r = rows[(rows[:, 0] == o.start[1] * ns + o.start[0]) & (rows[:, 1] == o.hole)]
    assert len(r) == 1, (o, len(r))
    return r[0]


def tier2_blocks(step):
    """blocks of MID_BLOCK steps tier 2 needs for a walk of `step` steps (LeanWalk::step, column 7 of a row): it ends in tier 2
    exactly when mid_steps, a whole number of blocks, is at least MID_BLOCK times this"""
    return (int(step) + MID_BLOCK - 1) // MID_BLOCK


def rule_starts(starts_lib, rows, binary):
    """the rows whose start the binarise kernels hand to the followers: the border-start rule of starts_core.h, spelt out pixel
    by pixel by tests/emul/starts_emul.cpp::se_rule (test_starts_cpu.build_lib), on the binary image with its frame zeroed"""
    b = np.ascontiguousarray((np.asarray(binary) > 0).astype(np.uint8))
    b[0, :] = b[-1, :] = 0
    b[:, 0] = b[:, -1] = 0
    sh, sw = b.shape
    ns = (sw + 15) & ~15
    out = np.zeros(b.size + 1, np.uint32)
    n = starts_lib.se_rule(P(b), sw, sh, P(out), out.size)
    assert 0 <= n <= out.size
    code = ((rows[:, 0] // ns) * sw + rows[:, 0] % ns).astype(np.uint32) | (rows[:, 1].astype(np.uint32) << np.uint32(31))
    keep = np.isin(code, out[:n])
    assert int(keep.sum()) == n, (int(keep.sum()), n)   # (every rule start is a plausible start)
    return rows[keep]


SHORT_STEPS = 96   # kernels.h: tier 1's probe


def straight_starts(lib, starts_lib, binary):
    """Tier 1 (follow.hip::follow_short) sends a frame's border that has at most two corner points after SHORT_STEPS steps
    straight to tier 3, whatever tier 2's budget (`if (lt.status == TRACE_OVERRUN) return lt.npts <= 2 ? 2 : 1;` at the end of
    follow_short's probe, route 2): the starts handed to the followers of which trace_flat says so, as rows of
    (position, is_hole, status, points, steps).  (Tier 1's look behind could still drop one: not the frame's own border at
    (1, 1), the first pixel of the scan.)"""
    b = np.ascontiguousarray((np.asarray(binary) > 0).astype(np.uint8))
    sh, sw = b.shape
    short = np.zeros((1 << 17, 8), np.int32)
    n = lib.fe_budget_walks(P(b), sw, sh, SHORT_STEPS, SHORT_STEPS, P(short), len(short))
    assert 0 <= n <= len(short)
    handed = rule_starts(starts_lib, short[:n], binary)   # (columns 0 .. 4 as fe_walks')
    return handed[(handed[:, 2] == 3) & (handed[:, 3] <= 2)][:, :5]


def budget_case(lib, starts_lib):
    """For the test that places tier 2's budget: the first 640x480 scene and owning border such that every walk handed to the
    followers whose step count lies in the border's own block of steps is a closed border (a walk that is not its border's
    first position may be dropped by tier 1's look behind, so whether tier 2 sees it is not known here).  Returns (scene,
    budget one block short, budget that covers it, walks that end in that block)."""
    for s in SCENES:
        if (s.w, s.h) != (640, 480):
            continue
        a = analyse(s.make())
        rows = walk_rows(lib, a.binary)
        handed = rule_starts(starts_lib, rows, a.binary)
        for o in a.owners:
            blocks = tier2_blocks(owner_row(rows, o, a.binary.shape[1])[7])
            inside = handed[(handed[:, 7] > MID_BLOCK * (blocks - 1)) & (handed[:, 7] <= MID_BLOCK * blocks)]
            # (sawtoothed all round: tier 1, which sends a border that barely turns in its first steps straight to tier 3, does
            # not take them)
            if len(inside) and (inside[:, 5] == 0).all() and (inside[:, 6] >= 500).all():
                return s, MID_BLOCK * (blocks - 1), MID_BLOCK * blocks, len(inside)
    raise AssertionError("no 640x480 scene whose owning border shares its block of steps with closed borders only")


def key_branch(o):
    return "key32" if o.n <= SLAB_PTS and o.diag2 < KEY32_DIAG2 else "key64"


def tier2_marks(lib, binary, o):
    """the corner points owning border o has completed after every block of MID_BLOCK steps of tier 2's walk (fe_tier2_marks of
    tests/emul/follow_emul.cpp): follow_mid_kernel flushes marks[i] - marks[i - 1] parked points after block i, up to SLAB_PTS"""
    b = np.ascontiguousarray((np.asarray(binary) > 0).astype(np.uint8))
    sh, sw = b.shape
    out = np.zeros(4 * b.size // MID_BLOCK + 2, np.int32)
    n = lib.fe_tier2_marks(P(b), sw, sh, o.start[1] * ((sw + 15) & ~15) + o.start[0], o.hole, P(out), len(out))
    assert n > 0 and out[n - 1] == o.n, (o, n)
    return [int(m) for m in out[:n]]


def tier2_flushes(marks):
    """the points of every flush: what the block produced, cut at the slab's end"""
    stored = np.minimum(np.concatenate([[0], marks]), SLAB_PTS)
    return np.diff(stored), np.diff(np.concatenate([[0], marks]))


def tier2_seams(marks, n):
    """the first point of every flush of tier 2 but the first one, on a border that tier 2 finishes from its slab"""
    return sorted({m for m in marks if 0 < m < n}) if n <= SLAB_PTS else []


def seam_indices(n, marks=()):
    """the indices either side of every seam a border of n points has: s - 1 and s, as far as the border has them, for
    s = 64, 128, ... <= n, 1024, 8192 and tier 2's flush seams"""
    out = set()
    for s in list(range(64, n + 1, 64)) + [SLAB_PTS, SLAB3_PTS] + tier2_seams(marks, n):
        out.update(i for i in (s - 1, s) if i < n)
    return sorted(out)


def tier2_classes(o, marks):
    """the classes owning border o reaches in follow_mid_kernel's parking and flushing"""
    flushed, produced = tier2_flushes(marks)
    assert (produced >= 0).all() and (produced <= MID_BLOCK).all() and int(flushed.sum()) == min(o.n, SLAB_PTS)
    if o.n > SLAB_PTS:
        i = int(np.flatnonzero(np.asarray(marks) > SLAB_PTS)[0])
        return {"t2cut=%d/%d" % (flushed[i], produced[i])}
    out = {"t2last=%d" % flushed[-1]}
    if (flushed == MID_BLOCK).any():
        out.add("t2full")
    seams = tier2_seams(marks, o.n)
    if any(i in seams or i + 1 in seams for idx in o.vertex_index for i in idx):
        out.add("vertex@t2flush")
    return out


def classes_of(o):
    """the classes owning border o reaches"""
    out = {"n=%d" % o.n, "n%%64=%d" % (o.n % 64), key_branch(o), "diag2=%d" % o.diag2}
    if o.n <= SLAB_PTS and o.diag2 >= KEY32_DIAG2:
        out.add("key64:box")
    if o.n > SLAB_PTS and 4 * o.diag2 < KEY32_DIAG2:
        out.add("key64:n")
    for idx in o.vertex_index:
        for name, s in SEAMS.items():
            for i in idx:
                if i >= s - 1 and (i % s == 0 or i % s == s - 1) and (name == "vertex@64" or i in (s - 1, s)):
                    out.add(name)
    return out

"""A second, plain reference of the middle of the path -- grey, pyrDown, pyrUp, adaptive threshold, border following, polygon
approximation and the square filter -- written from SURVEY.md Appendix A.1 to A.9 and from the topological definition of a
border, in numpy, scipy and plain Python.  It shares no code with oracle/ or with any *_core.h and loads no library of the
project: tests/test_plain_ref_cpu.py holds the oracle to it, tests/test_gpu_plain_ref.py the kernels.

Integer stages run in int64.  The polygon stage runs in Python ints and rationals, so it is exact where an implementation
rounds, and it says where a decision of A.7 is too close for roundings to be trusted (a *knife edge*, see approx)."""
from fractions import Fraction
from math import gcd

import numpy as np
from scipy import ndimage

# directions s = 0 .. 7 = E, NE, N, NW, W, SW, S, SE (A.5: increasing s turns counter-clockwise on the screen)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)
KNIFE = Fraction(1, 2 ** 45)


# ---- A.1 -----------------------------------------------------------------------------------------------------------------------
def grey(frame, fmt):
    """the grey image of a frame [H, W] or [H, W, bpp] in format "bgr", "rgb", "bgra", "rgba" or "gray\""""
    f = np.asarray(frame).astype(np.int64)
    if fmt == "gray":
        return f.reshape(f.shape[0], f.shape[1]).astype(np.uint8)
    blue, red = {"bgr": (0, 2), "bgra": (0, 2), "rgb": (2, 0), "rgba": (2, 0)}[fmt]
    return ((f[..., blue] * 1868 + f[..., 1] * 9617 + f[..., red] * 4899 + 8192) >> 14).astype(np.uint8)


# ---- A.2 to A.4 ----------------------------------------------------------------------------------------------------------------
def _pyr_down(roi):
    k = np.array([1, 4, 6, 4, 1], np.int64)
    rows = ndimage.correlate1d(roi, k, axis=1, mode="mirror")[:, ::2]      # 'mirror' is BORDER_REFLECT_101
    return (ndimage.correlate1d(rows, k, axis=0, mode="mirror")[::2] + 128) >> 8


def _up_axis(s, axis):
    """one direction of pyrUp: even outputs prev + 6 this + next, odd ones 4 (this + next); the neighbour before the first
    sample is the second sample, the neighbour behind the last one is the last one itself"""
    n = s.shape[axis]
    at = np.arange(n)
    before = np.where(at == 0, min(1, n - 1), at - 1)
    behind = np.where(at == n - 1, n - 1, at + 1)
    this, prev, nxt = s, np.take(s, before, axis), np.take(s, behind, axis)
    shape = list(s.shape)
    shape[axis] = 2 * n
    out = np.zeros(shape, np.int64)
    even = [slice(None)] * s.ndim
    odd = list(even)
    even[axis], odd[axis] = slice(0, None, 2), slice(1, None, 2)
    out[tuple(even)] = prev + 6 * this + nxt
    out[tuple(odd)] = 4 * (this + nxt)
    return out


def binarise(grey_image):
    """(binary, up) of the even-sized ROI of a grey image: the 0 / 255 result of the adaptive threshold, and the image after
    pyrDown and pyrUp that the threshold is taken of"""
    g = np.asarray(grey_image).astype(np.int64)
    roi = g[:g.shape[0] & ~1, :g.shape[1] & ~1]
    up = (_up_axis(_up_axis(_pyr_down(roi), 1), 0) + 32) >> 6
    k = np.array([8, 28, 56, 72, 56, 28, 8], np.int64)
    blur = ndimage.correlate1d(ndimage.correlate1d(up, k, axis=1, mode="nearest"), k, axis=0, mode="nearest")
    mean = (blur + 32768) >> 16
    return np.where(up > mean - 8, 255, 0).astype(np.uint8), up.astype(np.uint8)


# ---- A.5, from the definition: borders as what lies between a component and the background next to it --------------------------
def framed(binary):
    """0 / 1 image with the one-pixel frame zeroed"""
    b = (np.asarray(binary) > 0).astype(np.uint8)
    b[0, :] = b[-1, :] = 0
    b[:, 0] = b[:, -1] = 0
    return b


def borders(binary):
    """one record per border of a binary image, from connected-component labels alone: {(start, hole): (visited, filled)}.
    An outer border belongs to an 8-connected component of ones and starts at its first pixel in raster order; a hole border
    belongs to a 4-connected component of zeros other than the frame's and starts at *its* first pixel.  start = y * w + x.
    visited is the frozenset of y * w + x of the ones the border passes through: the pixels of the component of ones with a
    4-neighbour in the component of zeros on the border's other side.  filled (outer borders; None for holes) counts the pixels
    on or inside the border: the component with everything it encloses."""
    b = framed(binary)
    h, w = b.shape
    ones, n_ones = ndimage.label(b, structure=np.ones((3, 3), int))
    zeros, n_zeros = ndimage.label(1 - b)
    pairs = {}     # (label of ones, label of zeros) -> pixels of the first that touch the second
    ys, xs = np.nonzero(b)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        z = zeros[ys + dy, xs + dx]       # (a one is never on the frame, so the neighbour exists)
        m = z > 0
        for o, zz, p in zip(ones[ys[m], xs[m]].tolist(), z[m].tolist(), (ys[m] * w + xs[m]).tolist()):
            pairs.setdefault((o, zz), set()).add(p)
    out = {}
    first = np.unique(ones.ravel(), return_index=True)
    boxes = ndimage.find_objects(ones)
    for lab, at in zip(first[0].tolist(), first[1].tolist()):
        if lab == 0:
            continue
        y, x = divmod(at, w)
        body = np.pad(ones[boxes[lab - 1]] == lab, 1)
        outside = ndimage.label(~body)[0]
        filled = int(body.size - np.count_nonzero(outside == outside[0, 0]))
        out[(at, 0)] = (frozenset(pairs[(lab, int(zeros[y, x - 1]))]), filled)
    first = np.unique(zeros.ravel(), return_index=True)
    for lab, at in zip(first[0].tolist(), first[1].tolist()):
        if lab == 0 or lab == zeros[0, 0]:
            continue
        y, x = divmod(at, w)
        out[(at, 1)] = (frozenset(pairs[(int(ones[y, x - 1]), lab)]), None)
    return out


# ---- A.5, as a walk ------------------------------------------------------------------------------------------------------------
def _walk(img, w, x, y, hole):
    """A.5 step 3 from pixel (x, y): the CHAIN_APPROX_SIMPLE vertices of one border; labels the pixels it passes in img"""
    step = [DY[s] * w + DX[s] for s in range(8)]
    at0 = y * w + x
    s = last = 0 if hole else 4
    while True:
        s = (s - 1) & 7
        if img[at0 + step[s]] or s == last:
            break
    if s == last:
        img[at0] = -126
        return [(x, y)]
    second, at, came, pts = at0 + step[s], at0, s ^ 4, []
    while True:
        last = s
        while True:
            s += 1
            nxt = at + step[s & 7]
            if img[nxt]:
                break
        if s > 8:                        # the scan went past east (s = 8) and on: the pixel's east neighbour is zero
            img[at] = -126
        elif img[at] == 1:
            img[at] = 2
        s &= 7
        if s != came:
            pts.append((x, y))
            came = s
        x, y = x + DX[s], y + DY[s]
        if nxt == at0 and at == second:
            return pts
        at, s = nxt, (s + 4) & 7


def trace(binary):
    """every border of a binary image, followed as A.5 says, in list order (the border found last comes first):
    [(points [n, 2] int64 as x, y; start = y * w + x of the scan position; hole flag)]"""
    b = framed(binary)
    h, w = b.shape
    img = b.astype(np.int64).ravel().tolist()
    found = []
    # a border can only start where a row of the image changes between zero and non-zero: labels never change that
    change = np.flatnonzero(b[:, 1:w - 1].ravel() != b[:, 0:w - 2].ravel())
    for k in change.tolist():
        y, x = divmod(k, w - 2)
        x += 1
        if y == 0 or y == h - 1:
            continue
        prev, p = img[y * w + x - 1], img[y * w + x]
        if prev == 0 and p == 1:
            found.append((np.array(_walk(img, w, x, y, False), np.int64).reshape(-1, 2), y * w + x, 0))
        elif p == 0 and prev >= 1:
            found.append((np.array(_walk(img, w, x - 1, y, True), np.int64).reshape(-1, 2), y * w + x, 1))
    return found[::-1]


def pixels_of(pts):
    """the pixels a closed border passes, in order, from its CHAIN_APPROX_SIMPLE vertices: [(x, y)], one per step (a border of
    one point: that point)"""
    pts = [(int(p[0]), int(p[1])) for p in pts]
    if len(pts) == 1:
        return pts
    out = []
    for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
        n = max(abs(x1 - x0), abs(y1 - y0))
        assert n > 0 and (x1 - x0) % n == 0 and (y1 - y0) % n == 0 and (abs(x1 - x0) in (0, n)) and (abs(y1 - y0) in (0, n)), (
            "vertices not joined by a run of one of the 8 directions", (x0, y0), (x1, y1))
        out += [(x0 + (x1 - x0) // n * i, y0 + (y1 - y0) // n * i) for i in range(n)]
    return out


def lattice_points_on(pts):
    """B of Pick's theorem: the sum of gcd(|dx|, |dy|) over the edges of a closed polygon"""
    pts = [(int(p[0]), int(p[1])) for p in pts]
    return sum(gcd(abs(b[0] - a[0]), abs(b[1] - a[1])) for a, b in zip(pts, pts[1:] + pts[:1])) if len(pts) > 1 else 0


# ---- A.6 to A.8 ----------------------------------------------------------------------------------------------------------------
def arc_length(pts):
    """A.6: the closed perimeter, a float32 square root per edge, summed in double"""
    pts = [(int(p[0]), int(p[1])) for p in pts]
    if len(pts) <= 1:
        return 0.0
    total = 0.0
    for a, b in zip(pts[-1:] + pts[:-1], pts):
        dx, dy = np.float32(b[0]) - np.float32(a[0]), np.float32(b[1]) - np.float32(a[1])
        total += float(np.sqrt(np.float32(dx * dx) + np.float32(dy * dy)))
    return total


class _Decide:
    """comparisons lhs <= rhs of A.7, each made twice: as the definition rounds, and exactly"""

    def __init__(self):
        self.knife = False

    def le(self, rounded, lhs, rhs):
        """rounded: the decision in the definition's arithmetic; lhs, rhs: the same two sides as exact rationals"""
        big = max(abs(lhs), abs(rhs))
        if big > 0 and abs(lhs - rhs) < KNIFE * big:
            self.knife = True
        else:
            assert rounded == (lhs <= rhs), ("a rounded decision against the exact one, away from a knife edge", lhs, rhs)
        return rounded


def approx(pts, eps):
    """A.7 on a closed integer contour, in the variant of OpenCV <= 2.4.3 (the parity definition): the
    accuracy arrives as a float32 and is squared in float32 -- two roundings that the definition fixes, since each is one IEEE
    operation on given operands.  Every comparison against it is then made twice: in doubles, as the definition says, and in
    rationals from that same squared accuracy.  A decision whose exact sides differ by less than 2^-45 relative (both zero:
    decided) is a knife edge: each side takes at most four double roundings of 2^-53, and the margin keeps this reference from
    disagreeing with a correct implementation over the order of its multiplications.  Returns (polygon [m, 2] int64, whether
    any decision was a knife edge); the polygon follows the double decisions."""
    pts = [(int(p[0]), int(p[1])) for p in pts]
    n = len(pts)
    if n == 0:
        return np.zeros((0, 2), np.int64), False
    e = np.float32(eps)
    e2 = float(np.float32(e * e))     # float32, held in a double: exact
    e2x = Fraction(e2)
    d = _Decide()

    # 1. the seed: three times to the point farthest from the current one
    start, far, small = 0, 0, False
    for _ in range(3):
        start = (start + far) % n
        sx, sy = pts[start]
        best = 0
        for j in range(1, n):
            px, py = pts[(start + j) % n]
            dist = (px - sx) ** 2 + (py - sy) ** 2
            if dist > best:
                best, far = dist, j
        small = d.le(bool(np.float32(best) <= np.float32(e2)), Fraction(int(np.float32(best))), e2x)
    out = []
    if small:
        out.append(pts[start])
    else:
        # 2. two slices, in indices that may run past n (points are read modulo n)
        stack = [(start + far, start + n), (start, start + far)]
        # 3. split at the farthest point until every slice is within the accuracy
        while stack:
            a, b = stack.pop()
            sx, sy = pts[a % n]
            ex, ey = pts[b % n]
            keep = True
            if b > a + 1:
                dx, dy = ex - sx, ey - sy
                best, cut = 0, a
                for i in range(a + 1, b):
                    px, py = pts[i % n]
                    dist = abs((py - sy) * dx - (px - sx) * dy)
                    if dist > best:
                        best, cut = dist, i
                chord = dx * dx + dy * dy
                keep = d.le(float(best) * float(best) <= e2 * (float(dx) * float(dx) + float(dy) * float(dy)),
                            Fraction(best * best), e2x * chord)
            if keep:
                out.append((sx, sy))
            else:
                stack.append((cut, b))
                stack.append((a, cut))

    # 4. the clean-up pass over the ring of output points
    cnt = new_cnt = len(out)
    ring = list(out)
    r = cnt - 1
    start_pt = ring[r % cnt]
    r += 1
    wr = r % cnt
    pt = ring[r % cnt]
    r += 1
    i = 0
    while i < cnt and new_cnt > 2:
        end = ring[r % cnt]
        r += 1
        dx, dy = end[0] - start_pt[0], end[1] - start_pt[1]
        dist = abs((pt[0] - start_pt[0]) * dy - (pt[1] - start_pt[1]) * dx)
        chord = dx * dx + dy * dy
        if dx != 0 and dy != 0 and d.le(float(dist) * float(dist) <= 0.5 * e2 * float(chord), Fraction(dist * dist), e2x * chord / 2):
            new_cnt -= 1
            ring[wr] = start_pt = end
            wr = (wr + 1) % cnt
            pt = ring[r % cnt]
            r += 1
            i += 2
            continue
        ring[wr] = start_pt = pt
        wr = (wr + 1) % cnt
        pt = end
        i += 1
    return np.array(ring[:new_cnt], np.int64).reshape(-1, 2), d.knife


def area(pts):
    """A.8: the shoelace area of a closed polygon, signed, as a Fraction"""
    pts = [(int(p[0]), int(p[1])) for p in pts]
    return Fraction(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(pts[-1:] + pts[:-1], pts)), 2)


def is_convex(pts):
    """A.8: the cross products of consecutive edges are all strictly of one sign (a zero: not convex)"""
    pts = [(int(p[0]), int(p[1])) for p in pts]
    n = len(pts)
    if n == 0:
        return False
    cross = []
    for i in range(n):
        a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
        cross.append((b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]))
    return all(v > 0 for v in cross) or all(v < 0 for v in cross)


def polygon_of(pts):
    """what cvarFindSquares makes of one contour: approx at 0.02 of its perimeter -> (polygon, knife edge)"""
    return approx(pts, arc_length(pts) * 0.02)


def find_squares(grey_image, contours=None):
    """cvarFindSquares on a grey image -> (squares [k, 4, 2] int64 in list order, starts of the squares' borders [k] as
    y * sw + x | hole << 31, the same codes of the contours that could not be decided: a knife edge somewhere in them).
    A contour is kept with 4 vertices, |area| > 500, convex, and vertex 0 inside 2 < x < W - 2, 2 < y < H - 2 of the image
    itself (not of its even-sized ROI).  contours: trace() of the image's binarise(), when the caller has it already."""
    g = np.asarray(grey_image)
    H, W = g.shape
    if contours is None:
        contours = trace(binarise(g)[0])
    squares, starts, undecided = [], [], []
    for pts, start, hole in contours:
        code = start | hole << 31
        poly, knife = polygon_of(pts)
        if knife:
            undecided.append(code)
            continue
        if len(poly) == 4 and abs(area(poly)) > 500 and is_convex(poly):
            x, y = int(poly[0][0]), int(poly[0][1])
            if 2 < x < W - 2 and 2 < y < H - 2:
                squares.append(poly)
                starts.append(code)
    return np.array(squares, np.int64).reshape(-1, 4, 2), starts, undecided


# ---- A.9 and the crop pass -----------------------------------------------------------------------------------------------------
def crop_rect(quad, W, H):
    """(x0, y0, w, h): the bounding box of a square from its least to its greatest coordinate, 5 pixels more on every side,
    cut to the W x H image (cvarSquare2Rect, the +-5 at its call site, cvSetImageROI's clipping)"""
    q = np.asarray(quad).reshape(4, 2)
    x0, y0 = max(int(q[:, 0].min()) - 5, 0), max(int(q[:, 1].min()) - 5, 0)
    x1, y1 = min(int(q[:, 0].max()) + 5, W), min(int(q[:, 1].max()) + 5, H)
    return x0, y0, x1 - x0, y1 - y0


def crop_squares(grey_image, quad):
    """find_squares on the grey crop of a square; the last of its squares is the candidate's patPoint"""
    H, W = np.asarray(grey_image).shape
    x0, y0, w, h = crop_rect(quad, W, H)
    return find_squares(np.asarray(grey_image)[y0:y0 + h, x0:x0 + w])

"""What the tests of the frame operations share: the format tables, frames with guard bytes in the row padding and around the
buffer, hand-made marker records, device copies, the byte-for-byte comparison, and the module fixture `oa` of the GPU tests
(`from frame_kit import oa  # noqa: F401` puts it into a test module)."""
import numpy as np
import pytest

FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "gray": 4}
BPP = {0: 3, 1: 3, 2: 4, 3: 4, 4: 1}
FMTS = list(FORMATS)
E_ARG = -2   # include/ocvar_hip.h: OCVAR_E_ARG
MARKER_DTYPE = np.dtype([("glMatrix", "<f8", (16,)), ("templateId", "<i4"), ("markerId", "<i4"), ("score", "<f8"),
                         ("square", "<f4", (8,)), ("aspectRatio", "<f8")], align=True)
assert MARKER_DTYPE.itemsize == 184
GUARD = 0xA5
LEAD = 64   # guard bytes in front of the first frame and behind the last one (a multiple of 4: the frames stay aligned)


def bpp_of(fmt):
    """bytes per pixel of a format given by name"""
    return BPP[FORMATS[fmt]]


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import opencv_ar_amd
    opencv_ar_amd.hip_lib()
    return opencv_ar_amd


def records(squares, template_ids=None, scores=None):
    """[k] marker records with the given squares (k x 8 or k x 4 x 2), template ids (default 0) and scores (default 1)"""
    sq = np.asarray(squares, np.float32).reshape(-1, 8)
    r = np.zeros(len(sq), MARKER_DTYPE)
    r["square"] = sq
    r["templateId"] = 0 if template_ids is None else template_ids
    r["score"] = 1.0 if scores is None else scores
    r["markerId"] = np.arange(len(sq))
    return r


def axis_square(x0, y0, w, h):
    """the axis-aligned square whose corners are the pixel centres (x0, y0) .. (x0 + w - 1, y0 + h - 1), corner 0 top-left, clockwise
    on screen"""
    return [x0, y0, x0 + w - 1, y0, x0 + w - 1, y0 + h - 1, x0, y0 + h - 1]


def hand_made_records(rng, n, slots, W, Hh, frame_corners=True):
    """[n, slots] records with every field filled: convex squares in and around the frame and, with frame_corners, the frame's
    corners as the first square"""
    sq = np.zeros((n * slots, 4, 2), np.float32)
    for k in range(n * slots):
        s, a = rng.uniform(8, 0.4 * Hh), rng.uniform(0, 2 * np.pi)
        c = np.array([rng.uniform(-5, W + 5), rng.uniform(-5, Hh + 5)])
        ang = a + np.arange(4) * np.pi / 2
        sq[k] = c + s / np.sqrt(2) * np.stack([np.cos(ang), np.sin(ang)], 1)
    r = records(sq, template_ids=rng.integers(0, 9, n * slots), scores=rng.integers(0, 2, n * slots))
    r["glMatrix"] = rng.normal(size=(n * slots, 16))
    r["aspectRatio"] = rng.uniform(0.5, 2, n * slots)
    if frame_corners:
        r["square"][0] = [0, 0, W - 1, 0, W - 1, Hh - 1, 0, Hh - 1]
    return r.reshape(n, slots)


class Frames:
    """n frames of height x width pixels in format fmt inside one guarded byte buffer: the first frame `lead` bytes in, rows
    row_stride apart, frames frame_stride apart, LEAD bytes behind the last frame, every byte that is no pixel = GUARD.  `buf` is
    the whole buffer, `view(f)` frame f's [height, width, bpp] pixels; fill None: random pixels."""

    def __init__(self, n, width, height, fmt, row_pad=0, frame_gap=0, lead=LEAD, seed=0, fill=None):
        self.n, self.width, self.height, self.lead = n, width, height, lead
        self.fmt = FORMATS[fmt] if isinstance(fmt, str) else fmt
        self.bpp = BPP[self.fmt]
        self.row_stride = width * self.bpp + row_pad
        self.frame_stride = self.row_stride * height + frame_gap
        self.buf = np.full(lead + n * self.frame_stride + LEAD, GUARD, np.uint8)
        rng = np.random.default_rng(seed)
        for f in range(n):
            v = self.view(f)
            v[...] = rng.integers(0, 256, v.shape, dtype=np.uint8) if fill is None else fill

    def offset(self, f=0):
        return self.lead + f * self.frame_stride

    def view(self, f, buf=None):
        buf = self.buf if buf is None else buf
        return np.lib.stride_tricks.as_strided(buf[self.offset(f):], (self.height, self.width, self.bpp), (self.row_stride, self.bpp, 1))

    def pixel_mask(self):
        """True at every byte of the buffer that belongs to a pixel"""
        m = np.zeros(self.buf.size, bool)
        for f in range(self.n):
            self.view(f, m)[...] = True
        return m


def pix_layout(n, width, height, fmt, aligned, seed=0, fill=None):
    """frames for a case: aligned -- address, row stride and frame stride multiples of 4 (4 .. 7 bytes of row padding); else an odd
    lead, 1 byte of row padding and a frame gap of 5"""
    bpp = bpp_of(fmt)
    if aligned:
        p = Frames(n, width, height, fmt, row_pad=4 + (-width * bpp) % 4, frame_gap=8, lead=LEAD, seed=seed, fill=fill)
        assert p.row_stride % 4 == 0 and p.frame_stride % 4 == 0 and p.lead % 4 == 0
        return p
    return Frames(n, width, height, fmt, row_pad=1, frame_gap=5, lead=LEAD + 1, seed=seed, fill=fill)


def to_device(a, odd=False):
    """the bytes of a on the device; odd: one byte into an allocation (an odd address, allocations being aligned)"""
    import torch
    flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if not odd:
        return torch.from_numpy(flat).to("cuda:0")
    t = torch.zeros(flat.size + 1, dtype=torch.uint8, device="cuda:0")
    t[1:] = torch.from_numpy(flat).to("cuda:0")
    return t[1:]


def same(got, want, inside, where):
    """got and want are the same bytes; inside: the bool mask of the bytes that may change, or the layout (a Frames) whose
    pixel_mask() that is, which also places the first differing byte"""
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = "byte %d of the buffer" % bad[0]
        if not isinstance(inside, np.ndarray):
            lay, inside = inside, inside.pixel_mask()
            off = int(bad[0]) - lay.offset(0)
            at += " (frame %d row %d byte %d)" % (off // lay.frame_stride, off % lay.frame_stride // lay.row_stride,
                                                  off % lay.frame_stride % lay.row_stride)
        raise AssertionError("%s: %d bytes differ (%d of them guard bytes), first at %s: %d != %d" % (
            where, bad.size, int((~inside[bad]).sum()), at, got[bad[0]], want[bad[0]]))

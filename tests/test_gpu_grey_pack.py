"""GPU test of the frame binarise kernel's grey conversion in every colour format: the kernel keeps the grey value as byte 1 of
a 16-bit sum, two sums per register, and packs four of them with one byte permute (binarise.hip::to_grey; hd.h::grey_sum16 and
tests/test_grey_pack_cpu.py for the arithmetic).  The grey plane read back must be BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192)
>> 14, of every pixel -- on random pixels and on rows of the extremes -- for BGR, RGB, BGRA and RGBA frames of 512 x 30: three
strips, so a wave of an edge strip (reflected columns, byte loads) and a wave of an interior strip (the load plan) both run."""
import numpy as np
import pytest

from frame_kit import oa  # noqa: F401
from test_gpu_parity import make_detector
from test_gpu_starts import size

pytestmark = pytest.mark.gpu

W, HH, N = 512, 30, 3
EXTREMES = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255))   # (B, G, R)


@pytest.fixture(scope="module")
def bgr():
    """[3, 30, 512, 3] in B, G, R order: random pixels; rows 3 .. 7 of frame 0 and rows 20 .. 24 of frame 2 hold the extremes"""
    f = np.random.default_rng(2024).integers(0, 256, (N, HH, W, 3), np.uint8)
    for k, px in enumerate(EXTREMES):
        f[0, 3 + k] = px
        f[2, 20 + k] = px
    return f


@pytest.fixture(scope="module")
def want(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


@pytest.mark.parametrize("fmt", ["bgr", "rgb", "bgra", "rgba"])
def test_grey_plane_of_every_colour_format(oa, bgr, want, fmt):
    frames = bgr if fmt.startswith("bgr") else bgr[..., ::-1]
    if len(fmt) == 4:   # an alpha byte that changes from pixel to pixel: its weight is 0
        alpha = np.random.default_rng(7).integers(0, 256, (N, HH, W, 1), np.uint8)
        frames = np.concatenate([frames, alpha], axis=3)
    frames = np.ascontiguousarray(frames)
    det, _, _ = make_detector(oa, size(W, HH), None, N)
    det.set_input_format(fmt)
    det.detect_host(frames.copy())
    for f in range(N):
        got = det.debug_gray(f, W, HH)
        bad = np.argwhere(got != want[f])
        assert len(bad) == 0, (fmt, f, len(bad), bad[:4].tolist(), [int(got[tuple(p)]) for p in bad[:4]], [int(want[f][tuple(p)]) for p in bad[:4]])
    det.close()

"""Levels on the device (ocvar_hip_levels) byte for byte against the host build of levels_core.h (tests/levels_chain.py): whole
destination buffers are compared, the guard bytes in the row padding, between the planes and around the block included, and the
source is read back untouched every time."""
import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import levels_chain as LC
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401
from test_gpu_parity import OracleFrame, check_markers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return LC.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(64, 32, max_batch=1)   # (neither the sizes nor n_frames are bound by the context's)


def lib_params(oa, p):
    return None if p is None else oa.LevelsParams(*LC.as_tuple(p))


def device_levels(oa, det, src, dst, p=None, stream=None, d_src=None, d_dst=None, sync=True):
    """det.levels on device copies of src.buf and of dst.buf (or on the given ones) -> (destination buffer, source buffer afterwards)"""
    import torch
    d = to_device(src.buf) if d_src is None else d_src
    dd = to_device(dst.buf) if d_dst is None else d_dst
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.levels(d.data_ptr() + src.offset(0), dd.data_ptr() + dst.offset(0), src.width, src.height, src.n, params=lib_params(oa, p), fmt=src.fmt,
               src_row_stride=src.row_stride, src_frame_stride=src.frame_stride, dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride,
               stream=stream)
    if not sync:
        return dd, d
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


def check(oa, L, det, src, p, aligned, where, stream=None):
    """one call against the host core: the whole destination buffer, the source untouched -> the destination buffer"""
    dst = LC.dst_layout(src, aligned)
    rc, want = LC.host_levels(L, src, dst, p)
    assert rc == 0 and (want[~dst.pixel_mask()] == FK.GUARD).all()
    got, src_after = device_levels(oa, det, src, dst, p, stream=stream)
    assert (src_after == src.buf).all(), where
    same(got, want, dst.pixel_mask(), where)
    return got


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
def test_shapes_against_the_host_core(oa, L, det, fmt):
    """the CPU test's shapes and grids (37 x 23 under three grids, 1 x 1, 2 x 1, 5 x 3, one-pixel tiles, 8 x 8 on 16 x 16) under every
    setting of the knobs, 3 frames and one frame alone, on the dword path (everything a multiple of 4) and on the byte path (an odd
    lead, odd paddings, a frame gap of 5): the host core's buffer each time, the same pixels on both paths"""
    for k, (w, h, tiles) in enumerate(LC.SHAPES):
        for q, (lo, hi, gain) in enumerate(LC.KNOBS):
            p = LC.params(tiles, lo, hi, gain)
            n = 1 if (k + q) % 3 == 0 else 3
            pixels = []
            for aligned in (True, False):
                src = FK.pix_layout(n, w, h, fmt, aligned, seed=k + 1)
                got = check(oa, L, det, src, p, aligned, "%s %dx%d %s %s x %d aligned=%s" % (fmt, w, h, tiles, LC.KNOBS[q], n, aligned))
                dst = LC.dst_layout(src, aligned)
                pixels.append(np.stack([dst.view(f, got) for f in range(n)]))
            assert (pixels[0] == pixels[1]).all()


def test_default_params_are_the_null_pointer(oa, L, det):
    src = FK.pix_layout(2, 37, 23, "bgr", True, seed=3)
    a = check(oa, L, det, src, None, True, "params None")
    b = check(oa, L, det, src, LC.params(), True, "the defaults")
    assert (a == b).all()


@pytest.mark.parametrize("name", ["zeros", "mid", "ones", "two", "ramp", "halves"])
def test_special_frames(oa, L, det, name):
    """constant frames (every lane of the histogram kernel on one bin; both clamps of the gain cap), two values, the full range, lo
    above hi before the cap"""
    for w, h, tiles in [(37, 23, (1, 1)), (67, 41, (4, 3))]:
        g = LC.special_frames(w, h)[name]
        for fmt in ("gray", "bgr"):
            for lo, hi, gain in [LC.KNOBS[0], LC.KNOBS[2], LC.KNOBS[3]]:
                src = FK.pix_layout(2, w, h, fmt, True)
                for f in range(2):
                    src.view(f)[...] = g[:, :, None]
                check(oa, L, det, src, LC.params(tiles, lo, hi, gain), True, "%s %s %dx%d %s" % (name, fmt, w, h, tiles))


@pytest.mark.parametrize("fmt", ["gray", "bgr"])
def test_a_tile_of_several_row_slabs(oa, L, det, fmt):
    """64 x 300 with one tile: the histogram kernel's plan cuts a tile into slabs of LC.SLAB_ROWS = 32 rows, here ten of them, the
    last one of 12 rows; and with two tiles down the frame, whose slabs end inside the grid of workgroups"""
    assert -(-300 // LC.SLAB_ROWS) >= 3 and 300 % LC.SLAB_ROWS != 0
    for tiles in ((1, 1), (1, 2)):
        for aligned in (True, False):
            check(oa, L, det, FK.pix_layout(2, 64, 300, fmt, aligned, seed=4), LC.params(tiles), aligned, "slabs %s %s aligned=%s" % (fmt, tiles, aligned))


@pytest.mark.parametrize("tiles", [(4, 3), (8, 8)])
def test_grids_on_67_by_41(oa, L, det, tiles):
    for fmt in FK.FMTS:
        for aligned in (True, False):
            check(oa, L, det, FK.pix_layout(3, 67, 41, fmt, aligned, seed=5), LC.params(tiles), aligned, "67x41 %s %s aligned=%s" % (fmt, tiles, aligned))


def test_wider_than_one_segment(oa, L, det):
    """521 x 70 pixels: more than one segment of the apply kernel along x and along y inside a cell (LC.SEG_W = 256, LC.SEG_H = 32), with
    one tile and with a grid whose cells are cut too"""
    for tiles in ((1, 1), (2, 2), (3, 1)):
        for fmt, aligned in (("gray", True), ("bgr", False), ("bgra", True)):
            check(oa, L, det, FK.pix_layout(2, 521, 70, fmt, aligned, seed=6), LC.params(tiles), aligned, "521x70 %s %s" % (fmt, tiles))


# ---- rounds, streams, reuse ---------------------------------------------------------------------------------------------------------

def test_more_frames_than_one_round_takes(oa, L, det):
    """257 frames of 8 x 4: the workspace takes LC.WS_FRAMES = 256 a round"""
    assert LC.WS_FRAMES == 256
    for fmt, tiles in (("gray", (1, 1)), ("bgr", (2, 2))):
        check(oa, L, det, FK.pix_layout(257, 8, 4, fmt, True, seed=7), LC.params(tiles), True, "257 frames %s" % fmt)


def test_on_a_stream_of_the_caller(oa, L):
    import torch
    det = oa.Detector(64, 32, max_batch=1)
    s = torch.cuda.Stream()
    src = FK.pix_layout(3, 67, 41, "bgr", True, seed=8)
    check(oa, L, det, src, LC.params((4, 3)), True, "caller's stream", stream=s.cuda_stream)
    # two calls on two streams back to back: the library orders them on its workspace
    dst = LC.dst_layout(src, True)
    d, da, db = to_device(src.buf), to_device(dst.buf), to_device(dst.buf)
    torch.cuda.synchronize()
    kw = dict(fmt=src.fmt, src_row_stride=src.row_stride, src_frame_stride=src.frame_stride, dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride)
    pa, pb = LC.params((4, 3)), LC.params((2, 2), 0, 0, 512)
    det.levels(d.data_ptr() + src.offset(0), da.data_ptr() + dst.offset(0), 67, 41, 3, params=lib_params(oa, pa), stream=s.cuda_stream, **kw)
    det.levels(d.data_ptr() + src.offset(0), db.data_ptr() + dst.offset(0), 67, 41, 3, params=lib_params(oa, pb), stream=None, **kw)
    torch.cuda.synchronize()
    same(da.cpu().numpy(), LC.host_levels(L, src, dst, pa)[1], dst.pixel_mask(), "first of two streams")
    same(db.cpu().numpy(), LC.host_levels(L, src, dst, pb)[1], dst.pixel_mask(), "second of two streams")
    det.close()


def test_two_calls_back_to_back_with_different_grids(oa, L):
    """one context, one stream, nothing waited for in between: 8 x 8 tiles, then one tile, then 4 x 3 on other frames -- the LUT kernel
    leaves every histogram it has read zeroed, so each call counts from zero"""
    import torch
    det = oa.Detector(64, 32, max_batch=1)
    a, b = FK.pix_layout(3, 67, 41, "bgr", True, seed=9), FK.pix_layout(2, 37, 23, "gray", False, seed=10)
    calls = [(a, LC.params((8, 8)), True), (a, LC.params((1, 1)), True), (b, LC.params((4, 3)), False), (a, LC.params((8, 8)), True)]
    outs = [device_levels(oa, det, src, LC.dst_layout(src, al), p, sync=False)[0] for src, p, al in calls]
    torch.cuda.synchronize()
    for k, (src, p, al) in enumerate(calls):
        dst = LC.dst_layout(src, al)
        same(outs[k].cpu().numpy(), LC.host_levels(L, src, dst, p)[1], dst.pixel_mask(), "call %d of four" % k)
    det.close()


# ---- workspace and arguments ---------------------------------------------------------------------------------------------------------

def test_a_context_that_never_calls_levels_allocates_nothing(oa, L):
    """device memory in use: a context that turns and resizes frames but never calls levels holds what it held before; the first
    levels call of a context takes the workspace of 20 MiB (so the counter would have shown one), the second nothing.  The figure is
    the whole device's, so a difference is looked at again on a fresh context: another process's allocation does not repeat."""
    import torch
    src = FK.pix_layout(2, 64, 48, "bgr", True, seed=11)
    dst = LC.dst_layout(src, True)
    d, dd, turned = to_device(src.buf), to_device(dst.buf), to_device(np.zeros(2 * 64 * 48 * 3, np.uint8))
    warm = oa.Detector(64, 48, max_batch=1)      # (the process's first launches load the code object)
    device_levels(oa, warm, src, dst, None, d_src=d, d_dst=dd)
    warm.orient(d.data_ptr() + src.offset(0), 64, 48, turned.data_ptr(), 2, "rot180", fmt="bgr", src_row_stride=src.row_stride, src_frame_stride=src.frame_stride)
    torch.cuda.synchronize()
    for attempt in range(3):
        det = oa.Detector(64, 48, max_batch=1)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        det.orient(d.data_ptr() + src.offset(0), 64, 48, turned.data_ptr(), 2, "rot180", fmt="bgr", src_row_stride=src.row_stride, src_frame_stride=src.frame_stride)
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        if after == before:
            break
    assert after == before, (before, after)
    ws = LC.WS_BYTES
    for attempt in range(3):
        det = oa.Detector(64, 48, max_batch=1)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        device_levels(oa, det, src, dst, None, d_src=d, d_dst=dd)
        first = before - torch.cuda.mem_get_info()[0]
        device_levels(oa, det, src, dst, LC.params((4, 4)), d_src=d, d_dst=dd)
        second = before - torch.cuda.mem_get_info()[0]
        if first >= 0.9 * ws and second - first < ws // 2:
            break
    assert first >= 0.9 * ws and second - first < ws // 2, (first, second)


def test_refusals_launch_nothing(oa, L):
    import ctypes as C
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(32, 16, max_batch=1)
    ctx = det._ctx
    W, Hh, n = 64, 32, 2
    src_h = np.full(n * 4 * W * Hh + 64, 77, np.uint8)
    dst_h = np.full(n * 4 * W * Hh + 64, FK.GUARD, np.uint8)
    ds, dd = to_device(src_h), to_device(dst_h)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    sp, dp = ds.data_ptr(), dd.data_ptr()
    span = (2 ** 31) // (Hh - 1) + 1      # a row stride with which the rows span more than 2^31 - 1 bytes

    def call(**kw):
        a = dict(src=sp, w=W, h=Hh, srs=3 * W, fmt=0, dst=dp, drs=W, n=n, p=None)
        a.update(kw)
        p = a["p"]
        return lib.ocvar_hip_levels(ctx, a["src"], a["w"], a["h"], a["srs"], a.get("sfs", a["srs"] * max(a["h"], 1)), a["fmt"], a["dst"], a["drs"],
                                    a.get("dfs", a["drs"] * max(a["h"], 1)), a["n"], None if p is None else C.byref(oa.LevelsParams(*p)), None)

    cases = [dict(src=None), dict(dst=None), dict(fmt=5), dict(fmt=-1), dict(w=0), dict(h=0), dict(w=-1), dict(w=32768, srs=3 * 32768, drs=32768), dict(h=32768),
             dict(srs=3 * W - 1), dict(drs=W - 1), dict(fmt=2, srs=4 * W - 1), dict(fmt=4, srs=W - 1),
             dict(srs=span, sfs=3 * W * Hh, n=1), dict(drs=span, dfs=W * Hh, n=1), dict(n=0), dict(n=-1),
             dict(dst=sp), dict(dst=sp + 3 * W * Hh * n - 1), dict(src=dp + W * Hh * n - 1), dict(src=dp + 1),
             dict(p=(0, 1, 0, 0, 2048)), dict(p=(1, 0, 0, 0, 2048)), dict(p=(17, 1, 0, 0, 2048)), dict(p=(1, 17, 0, 0, 2048)), dict(p=(16, 5, 0, 0, 2048)),
             dict(p=(5, 1, 0, 0, 2048), w=4, srs=12, drs=4), dict(p=(1, 5, 0, 0, 2048), h=4),
             dict(p=(1, 1, -1, 0, 2048)), dict(p=(1, 1, 500001, 0, 2048)), dict(p=(1, 1, 0, -1, 2048)), dict(p=(1, 1, 0, 500001, 2048)),
             dict(p=(1, 1, 0, 0, 255)), dict(p=(1, 1, 0, 0, 65281)), dict(p=(1, 1, 0, 0, -5))]
    for rounds in range(2):
        for kw in cases:
            assert call(**kw) == E_ARG, kw
            assert lib.ocvar_hip_last_error(ctx).startswith(b"levels: "), kw
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == dst_h).all() and (ds.cpu().numpy() == src_h).all()
    assert torch.cuda.mem_get_info()[0] >= free_before - LC.WS_BYTES // 2      # (not even the workspace was taken)
    with pytest.raises(oa.OcvarError):
        det.levels(sp, sp, W, Hh, n, fmt="bgr")
    # after all that the context still works, on frames larger than its own maximum
    for p in (None, (4, 4, 0, 500000, 65280)):
        assert call(p=p) == 0
        torch.cuda.synchronize()
        want = dst_h.copy()
        hp = None if p is None else LC.Params(*p)      # (kept alive over the call)
        assert L.levels_emul(src_h.ctypes.data, W, Hh, 3 * W, 3 * W * Hh, 0, want.ctypes.data, W, W * Hh, n, None if hp is None else C.addressof(hp), None, None) == 0
        assert (dd.cpu().numpy() == want).all()


# ---- the chain on the device ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ["640x480", "320x240"])
def test_the_chain_on_the_device(oa, L, size):
    """the dark and the split exposures of the CPU chain's 640 x 480 and 320 x 240 scenes: levels on the device (one map per frame
    for dark, 4 x 4 tiles for split), then detection of the planes as GRAY input on the same stream with nothing waited for in
    between -- the planes are the host core's, and the records the oracle's on those planes, under the comparison of
    tests/test_gpu_parity.py"""
    import torch
    scenes = [bgr for name, bgr in LC.chain_scenes() if name.startswith(size)]
    h, w = scenes[0].shape[:2]
    tpls, cam = H.oracle_templates(), H.oracle_camera(w, h)
    n = 2 * len(scenes)
    frames = [LC.expose(bgr, "dark") for bgr in scenes] + [LC.expose(bgr, "split") for bgr in scenes]
    groups = [(0, len(scenes), LC.params()), (len(scenes), len(scenes), LC.params((4, 4)))]
    det = oa.Detector(w, h, max_batch=n)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    det.set_input_format("gray")
    d_src = to_device(np.stack(frames))
    d_planes = to_device(np.full(n * w * h, FK.GUARD, np.uint8))
    torch.cuda.synchronize()
    for f0, k, p in groups:
        det.levels(d_src.data_ptr() + f0 * w * h * 3, d_planes.data_ptr() + f0 * w * h, w, h, k, params=lib_params(oa, p), fmt="bgr")
    det.enqueue_device(d_planes.data_ptr(), w, h, n)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    assert (d_src.cpu().numpy().reshape(n, h, w, 3) == np.stack(frames)).all()
    planes = d_planes.cpu().numpy().reshape(n, h, w)
    found = 0
    for f0, k, p in groups:
        for f in range(f0, f0 + k):
            want = LC.host_levels_image(L, frames[f], p)
            assert (planes[f] == want).all(), (size, f, np.argwhere(planes[f] != want)[:4].tolist())
            ref = OracleFrame(np.repeat(want[:, :, None], 3, axis=2), tpls, cam, planes=False)
            check_markers(f, ref, markers, counts, where="levels chain %s" % size)
            found += len(ref.markers)
    assert found >= len(scenes)      # (the raw exposures yield no record at all: tests/test_levels_cpu.py)
    det.close()

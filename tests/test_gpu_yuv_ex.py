"""YUV conversion of every range, depth and layout on the device (ocvar_hip_yuv_to_frames_ex / ocvar_hip_frames_to_yuv_ex) byte for
byte against the host build of yuv_ex_core.h (tests/yuv_ex_chain.py): whole destination buffers are compared, the guard bytes in
the row padding, between the planes and the frames and around the block included."""
import ctypes as C

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import yuv_ex_chain as YX
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401
from test_gpu_parity import make_detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return YX.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(1026, 16, max_batch=1)   # (n_frames is not bound by the batch)


def yuv_struct(oa, yuv, base):
    st = yuv.struct(base)
    return oa.YuvFramesEx(st.layout, st.matrix, st.range, st.bits, st.y, st.c0, st.c1, st.y_pitch, st.c_pitch, st.frame_stride)


def device_to_frames(oa, det, yuv, dst):
    """det.yuv_to_frames on device copies of yuv.buf and of dst.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(yuv.buf), to_device(dst.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.yuv_to_frames(yuv_struct(oa, yuv, d.data_ptr()), dd.data_ptr() + dst.offset(0), yuv.width, yuv.height, yuv.n, fmt=dst.fmt,
                      dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


def device_to_yuv(oa, det, src, yuv):
    """det.frames_to_yuv on device copies of src.buf and of yuv.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(src.buf), to_device(yuv.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.frames_to_yuv(d.data_ptr() + src.offset(0), yuv_struct(oa, yuv, dd.data_ptr()), src.width, src.height, src.n, fmt=src.fmt,
                      src_row_stride=src.row_stride, src_frame_stride=src.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("layout,bits", YX.LAYOUT_DEPTHS)
def test_yuv_to_frames_sweep(oa, L, det, layout, bits, fmt):
    """every size with 2 frames, on the dword path (everything a multiple of 4) and on the byte path (an odd lead and odd paddings;
    16-bit samples: even ones that are no multiple of 4): the host core's buffer each time, and the same pixels on both paths"""
    for i, (W, Hh) in enumerate(YX.sizes_of(layout)):
        m, r = YX.variant(i)
        pixels = []
        for aligned in (True, False):
            yuv = YX.YuvEx(2, W, Hh, layout, bits, aligned=aligned, seed=W + Hh, matrix=m, rng=r)
            dst = FK.pix_layout(2, W, Hh, fmt, aligned, fill=FK.GUARD)
            want = YX.host_to_frames(L, yuv, dst, limit=1026)
            assert (want[~dst.pixel_mask()] == FK.GUARD).all()
            got, src_after = device_to_frames(oa, det, yuv, dst)
            assert (src_after == yuv.buf).all()
            same(got, want, dst.pixel_mask(), "%dx%d %s %d -> %s %s %s aligned=%s" % (W, Hh, layout, bits, fmt, m, r, aligned))
            pixels.append(np.stack([dst.view(f, got) for f in range(2)]))
        assert (pixels[0] == pixels[1]).all()


@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("layout,bits", YX.LAYOUT_DEPTHS)
def test_frames_to_yuv_sweep(oa, L, det, layout, bits, fmt):
    for i, (W, Hh) in enumerate(YX.sizes_of(layout)):
        m, r = YX.variant(i + 1)
        samples = []
        for aligned in (True, False):
            src = FK.pix_layout(2, W, Hh, fmt, aligned, seed=W * Hh)
            yuv = YX.YuvEx(2, W, Hh, layout, bits, aligned=aligned, matrix=m, rng=r)
            want = YX.host_to_yuv(L, src, yuv, limit=1026)
            assert (want[~yuv.sample_mask()] == FK.GUARD).all()
            got, src_after = device_to_yuv(oa, det, src, yuv)
            assert (src_after == src.buf).all()
            same(got, want, yuv.sample_mask(), "%dx%d %s -> %s %d %s %s aligned=%s" % (W, Hh, fmt, layout, bits, m, r, aligned))
            samples.append([yuv.samples(f, got) for f in range(2)])
        for f in range(2):
            assert all((p == q).all() for p, q in zip(samples[0][f], samples[1][f]))


# ---- stream order and chunks --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,bits,aligned", [("nv12", 10, True), ("nv12", 16, False), ("i444", 8, False), ("nv21", 8, True)])
def test_there_and_back_on_one_stream(oa, L, det, layout, bits, aligned):
    """frames_to_yuv and yuv_to_frames back, queued on the context's stream with nothing waited for in between"""
    import torch
    W, Hh, n = 514, 6, 3
    src = FK.pix_layout(n, W, Hh, "bgr", aligned, seed=9)
    yuv = YX.YuvEx(n, W, Hh, layout, bits, aligned=aligned, matrix="bt709", rng="full")
    back = FK.pix_layout(n, W, Hh, "bgra", aligned, fill=FK.GUARD)
    want_yuv = YX.host_to_yuv(L, src, yuv)
    want_back = YX.host_to_frames(L, yuv, back, buf=want_yuv)
    d, dy, db = to_device(src.buf), to_device(yuv.buf), to_device(back.buf)
    torch.cuda.synchronize()
    st = yuv_struct(oa, yuv, dy.data_ptr())
    det.frames_to_yuv(d.data_ptr() + src.offset(0), st, W, Hh, n, fmt="bgr", src_row_stride=src.row_stride, src_frame_stride=src.frame_stride)
    det.yuv_to_frames(st, db.data_ptr() + back.offset(0), W, Hh, n, fmt="bgra", dst_row_stride=back.row_stride, dst_frame_stride=back.frame_stride)
    torch.cuda.synchronize()
    same(dy.cpu().numpy(), want_yuv, yuv.sample_mask(), "to %s" % layout)
    same(db.cpu().numpy(), want_back, back.pixel_mask(), "and back")
    assert (back.view(0, want_back)[..., :3] != FK.GUARD).any()


def test_more_frames_than_one_launch_takes(oa, L, det):
    """65537 frames of 2 x 2 pixels of I444, stored without a gap: two launches (the grid's z ends at 65535), every frame converted
    once, in both directions"""
    import torch
    n, lead = 65537, 64
    rng = np.random.default_rng(2)
    yuv = np.full(lead + 12 * n + lead, FK.GUARD, np.uint8)     # per frame: Y Y / Y Y, U U / U U, V V / V V
    yuv[lead:lead + 12 * n] = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    pix = np.full(lead + 12 * n + lead, FK.GUARD, np.uint8)

    def st(base, matrix, rng_code):
        return YX.FramesEx(5, matrix, rng_code, 8, base + lead, base + lead + 4, base + lead + 8, 2, 2, 12)

    def dev(s):
        return oa.YuvFramesEx(5, s.matrix, s.range, 8, s.y, s.c0, s.c1, 2, 2, 12)

    want = pix.copy()
    s = st(yuv.ctypes.data, 2, 1)
    assert L.yuv_ex_to_frames_emul(C.addressof(s), want.ctypes.data + lead, 6, 12, 2, 2, n, 0, 1026, 16) == 0
    d, dd = to_device(yuv), to_device(pix)
    torch.cuda.synchronize()
    det.yuv_to_frames(dev(st(d.data_ptr(), 2, 1)), dd.data_ptr() + lead, 2, 2, n, fmt="bgr")
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:4].tolist()
    assert (got[lead + 12 * 65535: lead + 12 * n] != FK.GUARD).any()   # (the frames of the second launch)
    back = np.full(yuv.size, FK.GUARD, np.uint8)
    want_back = back.copy()
    s = st(want_back.ctypes.data, 0, 0)
    assert L.yuv_ex_from_frames_emul(want.ctypes.data + lead, 6, 12, C.addressof(s), 2, 2, n, 0, 1026, 16) == 0
    db = to_device(back)
    torch.cuda.synchronize()
    det.frames_to_yuv(dd.data_ptr() + lead, dev(st(db.data_ptr(), 0, 0)), 2, 2, n, fmt="bgr")
    torch.cuda.synchronize()
    assert (db.cpu().numpy() == want_back).all()


# ---- with detection ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,bits,m,r", [("nv12", 10, "bt709", "limited"), ("nv12", 8, "bt601", "full")])
def test_decoded_frames_are_converted_and_detected(oa, L, layout, bits, m, r):
    """one synthetic 640 x 480 scene as P010 BT.709 limited and as full-range NV12, made by the host core: converted on the device
    to BGR and to GRAY and detected -- the records of detection on the host core's converted frames, record for record"""
    import torch
    cfg = H.synth_config(2)
    W, Hh, n = cfg.width, cfg.height, 2
    det, tpls, cam = make_detector(oa, cfg, None, n)
    src = FK.pix_layout(n, W, Hh, "bgr", True)
    for f in range(n):
        src.view(f)[...] = H.synth_frame(cfg, f)[0]
    yuv = YX.YuvEx(n, W, Hh, layout, bits, aligned=True, matrix=m, rng=r)
    decoded = YX.host_to_yuv(L, src, yuv)                       # what the decoder delivers
    d = to_device(decoded)
    st = yuv_struct(oa, yuv, d.data_ptr())
    found = {}
    for fmt in ("bgr", "gray"):
        pix = FK.pix_layout(n, W, Hh, fmt, True, fill=FK.GUARD)
        want = YX.host_to_frames(L, yuv, pix, buf=decoded)
        dp, dw = to_device(pix.buf), to_device(want)
        torch.cuda.synchronize()
        det.set_input_format(fmt)
        det.yuv_to_frames(st, dp.data_ptr() + pix.offset(0), W, Hh, n, fmt=fmt, dst_row_stride=pix.row_stride, dst_frame_stride=pix.frame_stride)
        markers, counts = det.detect_device(dp.data_ptr() + pix.offset(0), W, Hh, n, row_stride=pix.row_stride, frame_stride=pix.frame_stride)
        markers, counts = markers.copy(), counts.copy()
        torch.cuda.synchronize()
        same(dp.cpu().numpy(), want, pix.pixel_mask(), "%s %d -> %s" % (layout, bits, fmt))
        ref_markers, ref_counts = det.detect_device(dw.data_ptr() + pix.offset(0), W, Hh, n, row_stride=pix.row_stride, frame_stride=pix.frame_stride)
        assert counts.min() >= 1 and (counts == ref_counts).all()
        for f in range(n):
            assert markers[f, :counts[f]].tobytes() == ref_markers[f, :counts[f]].tobytes(), (fmt, f)
        found[fmt] = (markers, counts)
    # GRAY is the library's grey of the converted colour: detection on it is detection on the converted BGR frame
    assert (found["bgr"][1] == found["gray"][1]).all()
    for f in range(n):
        k = found["bgr"][1][f]
        assert found["bgr"][0][f, :k].tobytes() == found["gray"][0][f, :k].tobytes()


# ---- refusals and the idle context --------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(64, 32, max_batch=1)
    ctx = det._ctx
    W, Hh, n = 64, 32, 2
    pix_h = np.full(n * 4 * W * Hh + 64, FK.GUARD, np.uint8)
    yuv_h = np.full(n * 6 * W * Hh + 64, 77, np.uint8)
    dp, dy = to_device(pix_h), to_device(yuv_h)
    torch.cuda.synchronize()
    pp, yp = dp.data_ptr(), dy.data_ptr()
    span = (2 ** 31) // (Hh - 1) + 1       # a pitch with which the rows of a plane span more than 2^31 - 1 bytes

    def call(to_frames, **kw):
        a = dict(layout=0, matrix=0, range=0, bits=8, y=yp, c0=yp + 2 * W * Hh, c1=yp + 4 * W * Hh, yp=W, cp=W, fs=6 * W * Hh, pix=pp, rs=3 * W,
                 w=W, h=Hh, n=n, fmt=0)
        a.update(kw)
        st = oa.YuvFramesEx(a["layout"], a["matrix"], a["range"], a["bits"], a["y"], a["c0"], a["c1"], a["yp"], a["cp"], a["fs"])
        ref = C.byref(st) if a.get("st", True) else None
        if to_frames:
            return lib.ocvar_hip_yuv_to_frames_ex(ctx, ref, a["pix"], a["rs"], a.get("pfs", a["rs"] * a["h"]), a["w"], a["h"], a["n"], a["fmt"], None)
        return lib.ocvar_hip_frames_to_yuv_ex(ctx, a["pix"], a["rs"], a.get("pfs", a["rs"] * a["h"]), ref, a["w"], a["h"], a["n"], a["fmt"], None)

    p010 = dict(bits=10, yp=2 * W, cp=2 * W)
    cases = [dict(st=False), dict(pix=None), dict(y=None), dict(c0=None), dict(layout=5, c1=None), dict(layout=4, c0=None),
             dict(layout=6), dict(layout=-1), dict(matrix=3), dict(matrix=-1), dict(range=2), dict(range=-1), dict(bits=9), dict(bits=0), dict(bits=17),
             dict(fmt=5), dict(fmt=-1), dict(p010, layout=1), dict(p010, layout=4), dict(p010, layout=5), dict(bits=16, layout=2),
             dict(w=W - 1), dict(layout=4, w=W - 1), dict(h=Hh - 1), dict(layout=4, h=Hh - 1), dict(w=W + 2), dict(h=Hh + 2), dict(layout=5, w=W + 1),
             dict(w=0), dict(h=0), dict(n=0), dict(n=-1), dict(yp=W - 1), dict(cp=W - 1), dict(layout=5, cp=W - 1), dict(p010, yp=2 * W - 2),
             dict(p010, cp=2 * W - 2), dict(p010, yp=2 * W + 1), dict(p010, cp=2 * W + 1), dict(p010, y=yp + 1), dict(p010, fs=6 * W * Hh + 1),
             dict(rs=3 * W - 1), dict(fmt=2, rs=4 * W - 1), dict(yp=span, n=1), dict(layout=5, cp=span, n=1), dict(rs=span, pfs=3 * W * Hh, n=1),
             dict(pix=yp), dict(pix=yp + W * Hh), dict(y=pp + 1), dict(c0=pp + 3 * W * Hh * n - 1), dict(layout=5, c1=pp + 8)]
    for to_frames in (True, False):
        for kw in cases:
            assert call(to_frames, **kw) == E_ARG, (to_frames, kw)
            assert lib.ocvar_hip_last_error(ctx), (to_frames, kw)
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == pix_h).all() and (dy.cpu().numpy() == yuv_h).all()
    # and after all that the context still converts: odd sides with I444, and P010
    assert call(True, layout=5, w=W - 1, h=Hh - 1, pfs=3 * W * Hh) == 0
    torch.cuda.synchronize()
    want = pix_h.copy()
    s = YX.FramesEx(5, 0, 0, 8, yuv_h.ctypes.data, yuv_h.ctypes.data + 2 * W * Hh, yuv_h.ctypes.data + 4 * W * Hh, W, W, 6 * W * Hh)
    assert L.yuv_ex_to_frames_emul(C.addressof(s), want.ctypes.data, 3 * W, 3 * W * Hh, W - 1, Hh - 1, n, 0, W, Hh) == 0
    assert (dp.cpu().numpy() == want).all()
    assert call(False, **p010) == 0
    torch.cuda.synchronize()
    want_y = yuv_h.copy()
    s = YX.FramesEx(0, 0, 0, 10, want_y.ctypes.data, want_y.ctypes.data + 2 * W * Hh, None, 2 * W, 2 * W, 6 * W * Hh)
    assert L.yuv_ex_from_frames_emul(want.ctypes.data, 3 * W, 3 * W * Hh, C.addressof(s), W, Hh, n, 0, W, Hh) == 0
    assert (dy.cpu().numpy() == want_y).all()


def test_the_calls_allocate_nothing(oa):
    """device memory in use is the same before and after the first _ex conversions of a context that has detected: no workspace.  A
    context of its own makes the first conversions of the process beforehand (the runtime loads a code object at its first launch).
    The figure is the whole device's, so a difference is looked at again on a fresh context: another process's allocation does not
    repeat, a workspace of these calls would."""
    import torch
    cfg = H.synth_config(2)
    W, Hh, n = cfg.width, cfg.height, 2
    frames = np.stack([H.synth_frame(cfg, f)[0] for f in range(n)])
    d = to_device(frames)
    dy = to_device(np.zeros(n * W * Hh * 3, np.uint8))
    dback = to_device(np.zeros(frames.size, np.uint8))
    sts = [oa.YuvFramesEx.from_surface(dy.data_ptr(), W, Hh, "nv12", bits=10, matrix="bt2020"),
           oa.YuvFramesEx.from_surface(dy.data_ptr(), W, Hh, "i444", range="full"), oa.YuvFramesEx.from_surface(dy.data_ptr(), W, Hh, "nv21")]
    assert (sts[0].c0, sts[0].y_pitch, sts[0].frame_stride) == (dy.data_ptr() + 2 * W * Hh, 2 * W, 3 * W * Hh)

    def convert(det):
        for st in sts:
            det.frames_to_yuv(d.data_ptr(), st, W, Hh, n)
            det.yuv_to_frames(st, dback.data_ptr(), W, Hh, n)
        torch.cuda.synchronize()

    convert(oa.Detector(W, Hh, max_batch=n))
    for attempt in range(3):
        det, tpls, cam = make_detector(oa, cfg, None, n)
        markers, counts = det.detect_device(d.data_ptr(), W, Hh, n)
        assert counts.min() >= 1
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        convert(det)
        after = torch.cuda.mem_get_info()[0]
        if after == before:
            break
    assert after == before, (before, after)
    assert (d.cpu().numpy() == frames.reshape(-1)).all() and dback.cpu().numpy().any()

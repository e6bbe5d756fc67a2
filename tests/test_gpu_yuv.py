"""YUV conversion on the device (ocvar_hip_yuv_to_frames / ocvar_hip_frames_to_yuv) byte for byte against the host build of
yuv_core.h (tests/yuv_chain.py): whole destination buffers are compared, the guard bytes in the row padding, between the planes
and the frames and around the block included."""
import ctypes as C

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import overlay_chain as OC
import yuv_chain as YC
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401
from test_gpu_parity import OracleFrame, check_markers, make_detector

pytestmark = pytest.mark.gpu

MATS = ["bt601", "bt709"]


@pytest.fixture(scope="module")
def L():
    return YC.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(1026, 16, max_batch=1)   # (n_frames is not bound by the batch)


def yuv_struct(oa, yuv, base, matrix):
    y, c0, c1 = yuv.pointers(base)
    return oa.YuvFrames(yuv.layout, YC.MATRICES[matrix], y, c0, c1, yuv.y_pitch, yuv.c_pitch, yuv.frame_stride)


def device_to_frames(oa, det, yuv, matrix, dst, buf=None):
    """det.yuv_to_frames on device copies of yuv.buf (or buf) and of dst.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(yuv.buf if buf is None else buf), to_device(dst.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.yuv_to_frames(yuv_struct(oa, yuv, d.data_ptr(), matrix), dd.data_ptr() + dst.offset(0), yuv.width, yuv.height, yuv.n, fmt=dst.fmt,
                      dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


def device_to_yuv(oa, det, src, matrix, yuv, buf=None):
    """det.frames_to_yuv on device copies of src.buf (or buf) and of yuv.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(src.buf if buf is None else buf), to_device(yuv.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.frames_to_yuv(d.data_ptr() + src.offset(0), yuv_struct(oa, yuv, dd.data_ptr(), matrix), src.width, src.height, src.n, fmt=src.fmt,
                      src_row_stride=src.row_stride, src_frame_stride=src.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


# ---- the layout sweep ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("layout", list(YC.LAYOUTS))
def test_yuv_to_frames_sweep(oa, L, det, layout, fmt):
    """every size with 1 and 3 frames, on the dword path (everything a multiple of 4) and on the byte path (an odd lead, odd
    paddings): the host core's buffer each time, and the same pixels on both paths"""
    for i, (W, Hh) in enumerate(YC.SIZES):
        m = MATS[i % 2]
        for n in (1, 3):
            pixels = []
            for aligned in (True, False):
                yuv = YC.Yuv(n, W, Hh, layout, aligned=aligned, seed=W + Hh)
                dst = FK.pix_layout(n, W, Hh, fmt, aligned, fill=FK.GUARD)
                want = YC.host_to_frames(L, yuv, m, dst)
                assert (want[~dst.pixel_mask()] == FK.GUARD).all()
                got, src_after = device_to_frames(oa, det, yuv, m, dst)
                assert (src_after == yuv.buf).all()
                same(got, want, dst.pixel_mask(), "%dx%d x %d %s -> %s %s aligned=%s" % (W, Hh, n, layout, fmt, m, aligned))
                pixels.append(np.stack([dst.view(f, got) for f in range(n)]))
            assert (pixels[0] == pixels[1]).all()


@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("layout", list(YC.LAYOUTS))
def test_frames_to_yuv_sweep(oa, L, det, layout, fmt):
    for i, (W, Hh) in enumerate(YC.SIZES):
        m = MATS[(i + 1) % 2]
        for n in (1, 3):
            samples = []
            for aligned in (True, False):
                src = FK.pix_layout(n, W, Hh, fmt, aligned, seed=W * Hh)
                yuv = YC.Yuv(n, W, Hh, layout, aligned=aligned)
                want = YC.host_to_yuv(L, src, m, yuv)
                assert (want[~yuv.sample_mask()] == FK.GUARD).all()
                got, src_after = device_to_yuv(oa, det, src, m, yuv)
                assert (src_after == src.buf).all()
                same(got, want, yuv.sample_mask(), "%dx%d x %d %s -> %s %s aligned=%s" % (W, Hh, n, fmt, layout, m, aligned))
                samples.append([yuv.samples(f, got) for f in range(n)])
            for f in range(n):
                assert all((p == q).all() for p, q in zip(samples[0][f], samples[1][f]))


# ---- stream order and chunks --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False])
def test_there_and_back_on_one_stream(oa, L, det, aligned):
    """frames_to_yuv into NV12 and yuv_to_frames back, queued on the context's stream with nothing waited for in between"""
    import torch
    W, Hh, n = 514, 6, 3
    src = FK.pix_layout(n, W, Hh, "bgr", aligned, seed=9)
    yuv = YC.Yuv(n, W, Hh, "nv12", aligned=aligned)
    back = FK.pix_layout(n, W, Hh, "bgra", aligned, fill=FK.GUARD)
    want_yuv = YC.host_to_yuv(L, src, "bt709", yuv)
    want_back = YC.host_to_frames(L, yuv, "bt709", back, buf=want_yuv)
    d, dy, db = to_device(src.buf), to_device(yuv.buf), to_device(back.buf)
    torch.cuda.synchronize()
    st = yuv_struct(oa, yuv, dy.data_ptr(), "bt709")
    det.frames_to_yuv(d.data_ptr() + src.offset(0), st, W, Hh, n, fmt="bgr", src_row_stride=src.row_stride, src_frame_stride=src.frame_stride)
    det.yuv_to_frames(st, db.data_ptr() + back.offset(0), W, Hh, n, fmt="bgra", dst_row_stride=back.row_stride, dst_frame_stride=back.frame_stride)
    torch.cuda.synchronize()
    same(dy.cpu().numpy(), want_yuv, yuv.sample_mask(), "to NV12")
    same(db.cpu().numpy(), want_back, back.pixel_mask(), "and back")
    # (the round trip of random pixels moves them: 4:2:0 averages their chroma)
    assert (back.view(0, want_back)[..., :3] != src.view(0)).any()


def test_more_frames_than_one_launch_takes(oa, L, det):
    """65537 frames of 2 x 2 pixels, stored without a gap: two launches (the grid's z ends at 65535), every frame converted once"""
    import torch
    n, lead = 65537, 64
    rng = np.random.default_rng(2)
    yuv = np.full(lead + 6 * n + lead, FK.GUARD, np.uint8)     # per frame: Y Y / Y Y / U V
    yuv[lead:lead + 6 * n] = rng.integers(0, 256, 6 * n, dtype=np.uint8)
    pix = np.full(lead + 12 * n + lead, FK.GUARD, np.uint8)
    want = pix.copy()
    L.yuv_to_frames_emul(0, 0, yuv.ctypes.data + lead, yuv.ctypes.data + lead + 4, None, 2, 2, 6, want.ctypes.data + lead, 6, 12, 2, 2, 0, n)
    d, dd = to_device(yuv), to_device(pix)
    torch.cuda.synchronize()
    det.yuv_to_frames(oa.YuvFrames(0, 0, d.data_ptr() + lead, d.data_ptr() + lead + 4, None, 2, 2, 6), dd.data_ptr() + lead, 2, 2, n, fmt="bgr")
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:4].tolist()
    assert (got[lead + 12 * 65535: lead + 12 * n] != FK.GUARD).any()   # (the frames of the second launch)
    back = np.full(yuv.size, FK.GUARD, np.uint8)
    want_back = back.copy()
    L.frames_to_yuv_emul(0, 1, want_back.ctypes.data + lead, want_back.ctypes.data + lead + 4, None, 2, 2, 6, want.ctypes.data + lead, 6, 12, 2, 2, 0, n)
    db = to_device(back)
    torch.cuda.synchronize()
    det.frames_to_yuv(dd.data_ptr() + lead, oa.YuvFrames(0, 1, db.data_ptr() + lead, db.data_ptr() + lead + 4, None, 2, 2, 6), 2, 2, n, fmt="bgr")
    torch.cuda.synchronize()
    assert (db.cpu().numpy() == want_back).all()


# ---- with detection ------------------------------------------------------------------------------------------------------------------

COLOUR = np.array([250, 10, 200, 255], np.uint8)   # R G B A


def test_decoded_frames_are_detected_drawn_on_and_encoded(oa, L):
    """the loop of a decoder's NV12 frames: converted on the device to BGR and to GRAY, each detected -- the oracle's registration on
    the host core's BGR bytes, and the same records from both; then the overlay drawn on the BGR frames and those converted to NV12
    -- the host cores of both steps"""
    import torch
    cfg = H.synth_config(2)   # 640 x 480, four markers: the size the synthetic scenes are made for
    W, Hh, n = cfg.width, cfg.height, 2
    det, tpls, cam = make_detector(oa, cfg, None, n)
    src = FK.pix_layout(n, W, Hh, "bgr", True)
    for f in range(n):
        src.view(f)[...] = H.synth_frame(cfg, f)[0]
    yuv = YC.Yuv(n, W, Hh, "nv12", aligned=True)
    nv12 = YC.host_to_yuv(L, src, "bt601", yuv)                 # what the decoder delivers
    bgr, gray = FK.pix_layout(n, W, Hh, "bgr", True, fill=FK.GUARD), FK.pix_layout(n, W, Hh, "gray", False, fill=FK.GUARD)
    want_bgr = YC.host_to_frames(L, yuv, "bt601", bgr, buf=nv12)
    d, db, dg = to_device(nv12), to_device(bgr.buf), to_device(gray.buf)
    torch.cuda.synchronize()
    st = yuv_struct(oa, yuv, d.data_ptr(), "bt601")
    LO = OC.build_emul()
    overlay = np.broadcast_to(COLOUR, (4, 4, 4)).copy()
    det.set_overlay(-1, overlay)
    out = YC.Yuv(n, W, Hh, "nv12", aligned=True)
    do = to_device(out.buf)
    torch.cuda.synchronize()
    # GRAY: convert, detect
    det.set_input_format("gray")
    det.yuv_to_frames(st, dg.data_ptr() + gray.offset(0), W, Hh, n, fmt="gray", dst_row_stride=gray.row_stride, dst_frame_stride=gray.frame_stride)
    det.enqueue_device(dg.data_ptr() + gray.offset(0), W, Hh, n, row_stride=gray.row_stride, frame_stride=gray.frame_stride)
    g_markers, g_counts = det.collect()
    g_markers, g_counts, g_greys = g_markers.copy(), g_counts.copy(), [det.debug_gray(f, W, Hh).copy() for f in range(n)]
    # BGR: convert, detect, draw on the frames behind the batch, convert what was drawn -- one stream, nothing waited for but the
    # snapshot of the converted frames
    det.set_input_format("bgr")
    det.yuv_to_frames(st, db.data_ptr() + bgr.offset(0), W, Hh, n, fmt="bgr", dst_row_stride=bgr.row_stride, dst_frame_stride=bgr.frame_stride)
    torch.cuda.synchronize()
    same(db.cpu().numpy(), want_bgr, bgr.pixel_mask(), "NV12 -> BGR")
    det.enqueue_device(db.data_ptr() + bgr.offset(0), W, Hh, n, row_stride=bgr.row_stride, frame_stride=bgr.frame_stride)
    det.render(db.data_ptr() + bgr.offset(0), W, Hh, fmt="bgr", row_stride=bgr.row_stride, frame_stride=bgr.frame_stride)
    det.frames_to_yuv(db.data_ptr() + bgr.offset(0), yuv_struct(oa, out, do.data_ptr(), "bt601"), W, Hh, n, fmt="bgr",
                      src_row_stride=bgr.row_stride, src_frame_stride=bgr.frame_stride)
    markers, counts = det.collect()
    greys = [det.debug_gray(f, W, Hh).copy() for f in range(n)]
    torch.cuda.synchronize()
    for f in range(n):
        ref = OracleFrame(np.ascontiguousarray(bgr.view(f, want_bgr)), tpls, cam, planes=True)
        assert len(ref.markers) >= 1
        check_markers(f, ref, markers, counts, where="bgr")
        assert np.array_equal(greys[f], ref.grey)
        assert np.array_equal(g_greys[f], ref.grey) and np.array_equal(gray.view(f, dg.cpu().numpy())[..., 0], ref.grey)
    assert g_markers.tobytes() == markers.tobytes() and (g_counts == counts).all()
    rendered, drawn = OC.host_render(LO, bgr, markers, counts, {-1: overlay}, buf=want_bgr)
    assert min(drawn) >= 1 and (rendered != want_bgr).any()
    same(db.cpu().numpy(), rendered, bgr.pixel_mask(), "rendered")
    same(do.cpu().numpy(), YC.host_to_yuv(L, bgr, "bt601", out, buf=rendered), out.sample_mask(), "rendered -> NV12")


# ---- refusals and the idle context --------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(64, 32, max_batch=1)
    ctx = det._ctx
    W, Hh, n = 64, 32, 2
    pix_h = np.full(n * 4 * W * Hh + 64, FK.GUARD, np.uint8)
    yuv_h = np.full(n * 2 * W * Hh + 64, 77, np.uint8)
    dp, dy = to_device(pix_h), to_device(yuv_h)
    torch.cuda.synchronize()
    pp, yp = dp.data_ptr(), dy.data_ptr()
    span = (2 ** 31) // (Hh - 1) + 1       # a pitch with which the rows of a plane span more than 2^31 - 1 bytes
    span_c = (2 ** 31) // (Hh // 2 - 1) + 1

    def call(to_frames, **kw):
        a = dict(layout=0, matrix=0, y=yp, c0=yp + W * Hh, c1=yp + W * Hh * 5 // 4, yp=W, cp=W, fs=W * Hh * 2, pix=pp, rs=3 * W, w=W, h=Hh, n=n, fmt=0)
        a.update(kw)
        st = oa.YuvFrames(a["layout"], a["matrix"], a["y"], a["c0"], a["c1"], a["yp"], a["cp"], a["fs"]) if a.get("st", True) else None
        ref = C.byref(st) if st is not None else None
        if to_frames:
            return lib.ocvar_hip_yuv_to_frames(ctx, ref, a["pix"], a["rs"], a.get("pfs", a["rs"] * a["h"]), a["w"], a["h"], a["n"], a["fmt"], None)
        return lib.ocvar_hip_frames_to_yuv(ctx, a["pix"], a["rs"], a.get("pfs", a["rs"] * a["h"]), ref, a["w"], a["h"], a["n"], a["fmt"], None)

    cases = [dict(st=False), dict(pix=None), dict(y=None), dict(c0=None), dict(layout=1, cp=W // 2, c1=None), dict(layout=1, cp=W // 2, c0=None),
             dict(layout=4), dict(layout=-1), dict(matrix=2), dict(matrix=-1), dict(fmt=5), dict(fmt=-1),
             dict(w=W - 1), dict(layout=2, yp=2 * W, w=W - 3), dict(h=Hh - 1), dict(layout=1, cp=W // 2, h=Hh - 1),
             dict(w=W + 2), dict(h=Hh + 2), dict(w=0), dict(h=0), dict(n=0), dict(n=-1),
             dict(yp=W - 1), dict(cp=W - 1), dict(layout=1, cp=W // 2 - 1), dict(layout=2, yp=2 * W - 1), dict(layout=3, yp=2 * W - 1),
             dict(rs=3 * W - 1), dict(fmt=2, rs=4 * W - 1), dict(fmt=4, rs=W - 1),
             dict(yp=span, n=1), dict(cp=span_c, n=1), dict(layout=1, cp=span_c, n=1), dict(layout=2, yp=span, n=1), dict(rs=span, pfs=3 * W * Hh, n=1),
             dict(pix=yp), dict(pix=yp + W * Hh * 2 * n - W * Hh // 2 - 1), dict(pix=yp + W * Hh), dict(y=pp + 1), dict(c0=pp + 3 * W * Hh * n - 1),
             dict(layout=1, cp=W // 2, c1=pp), dict(layout=3, yp=2 * W, y=pp + 3 * W * Hh * n - 1)]
    for to_frames in (True, False):
        for kw in cases:
            assert call(to_frames, **kw) == E_ARG, (to_frames, kw)
            assert lib.ocvar_hip_last_error(ctx), (to_frames, kw)
    # an odd height is no fault with a 4:2:2 layout, and a plane pointer the layout does not use may be anything
    assert call(True, layout=2, yp=2 * W, h=Hh - 1, c0=None, c1=None) == 0
    torch.cuda.synchronize()
    pix_after = dp.cpu().numpy()
    assert (pix_after[3 * W * (Hh - 1) * n:] == FK.GUARD).all() and (pix_after[:3 * W * (Hh - 1)] != FK.GUARD).any()
    dp.copy_(torch.from_numpy(pix_h))
    torch.cuda.synchronize()
    for to_frames in (True, False):
        for kw in cases:
            assert call(to_frames, **kw) == E_ARG
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == pix_h).all() and (dy.cpu().numpy() == yuv_h).all()
    # and after all that the context still converts
    assert call(True) == 0 and call(False) == 0
    torch.cuda.synchronize()
    got = dp.cpu().numpy()
    want = pix_h.copy()
    L.yuv_to_frames_emul(0, 0, yuv_h.ctypes.data, yuv_h.ctypes.data + W * Hh, None, W, W, W * Hh * 2, want.ctypes.data, 3 * W, 3 * W * Hh, W, Hh, 0, n)
    assert (got == want).all()


def test_the_calls_allocate_nothing(oa):
    """device memory in use is the same before and after the first conversions of a context that has detected: no workspace.  A
    context of its own makes the first conversions of the process beforehand (the runtime loads a code object at its first launch).
    The figure is the whole device's, so a difference is looked at again on a fresh context: another process's allocation does not
    repeat, a workspace of these calls would."""
    import torch
    cfg = H.synth_config(2)
    W, Hh, n = cfg.width, cfg.height, 2
    frames = np.stack([H.synth_frame(cfg, f)[0] for f in range(n)])
    d = to_device(frames)
    dy = to_device(np.zeros(n * W * Hh * 3 // 2, np.uint8))
    dback = to_device(np.zeros(frames.size, np.uint8))
    st = oa.YuvFrames.from_surface(dy.data_ptr(), W, Hh, "nv12")
    assert (st.c0, st.c1, st.y_pitch, st.c_pitch, st.frame_stride) == (dy.data_ptr() + W * Hh, None, W, W, W * Hh * 3 // 2)

    def convert(det):
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

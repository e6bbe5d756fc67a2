"""Bayer demosaic on the device (ocvar_hip_bayer_to_frames) byte for byte against the host build of bayer_core.h
(tests/bayer_chain.py), with no tolerance: whole destination buffers are compared, the guard bytes in the row padding, between the
frames and around the block included, and the source afterwards."""
import ctypes as C

import numpy as np
import pytest

import annotate_chain as AC
import bayer_chain as BC
import frame_kit as FK
import helpers as H
import levels_chain as LC
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401
from test_gpu_parity import OracleFrame, check_markers, make_detector

pytestmark = pytest.mark.gpu

PATS = list(BC.PATTERNS)
# The kernel's seams: a lane's span of 8 pixels, a wave's span of 512, the even-aligned row pair, and the strip of BC.PAIRS = 4 row
# pairs (8 rows) a lane marches down.  The widths are the two spans and their neighbours, 520 (a second workgroup of one full lane)
# and 1031 (three workgroups, the last lane of 7); the heights 2 .. 5 are both sides of the row pair (an odd height ends in a pair
# of one row), 7 .. 10 both sides of the strip (9: a second strip of one row), 17 is three strips, the last of one row.
WIDTHS = [2, 3, 7, 8, 9, 15, 16, 17, 511, 512, 513, 520, 1031]
HEIGHTS = [2, 3, 4, 5, 17, 7, 8, 9, 10]


@pytest.fixture(scope="module")
def L():
    return BC.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(64, 32, max_batch=1)   # (neither the sides nor n_frames are bound by the context)


def lib_params(oa, p):
    return None if p is None else oa.BayerParams(*BC.as_tuple(p))


def device_demosaic(oa, det, raw, dst, p, buf=None):
    """det.bayer_to_frames on device copies of raw.buf (or buf) and of dst.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(raw.buf if buf is None else buf), to_device(dst.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.bayer_to_frames(d.data_ptr() + raw.offset(0), dd.data_ptr() + dst.offset(0), raw.width, raw.height, raw.n, params=lib_params(oa, p), fmt=dst.fmt,
                        src_row_stride=raw.row_stride, src_frame_stride=raw.frame_stride, dst_row_stride=dst.row_stride,
                        dst_frame_stride=dst.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


def test_the_python_parameters(oa):
    p = oa.bayer_params()
    q = oa.BayerParams()
    assert oa.hip_lib().ocvar_hip_bayer_default_params(C.byref(q)) == 0
    assert BC.as_tuple(p) == BC.as_tuple(q) == (0, 8, 0, 1024, 1024, 1024) and C.sizeof(oa.BayerParams) == 24
    assert BC.as_tuple(oa.bayer_params("BGGR", 12, 64, (1.5, 1, 2))) == (3, 12, 64, 1536, 1024, 2048) and oa.BAYER_PATTERNS == BC.PATTERNS
    for kw in (dict(pattern="rgbg"), dict(pattern=4), dict(bits=7), dict(bits=17), dict(black=256), dict(black=-1), dict(gains=(1, 1)), dict(gains=(16, 1, 1)),
               dict(gains=(1, -0.1, 1))):
        with pytest.raises(ValueError):
            oa.bayer_params(**kw)
    assert [oa.bayer_pattern_at("rggb", x, y) for x, y in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 4))] == ["rggb", "grbg", "gbrg", "bggr", "rggb"]
    assert oa.hip_lib().ocvar_hip_bayer_pattern_at(4, 0, 0) == -1


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("pattern", PATS)
def test_sweep(oa, L, det, pattern, fmt):
    """every width, paired with a height that moves with the case, with 1 and 3 frames, from 8-bit and from 12-bit sources, on the
    dword path (everything a multiple of 4) and on the byte path (an odd lead and pitch; for words an even lead off a multiple of 4):
    the host core's buffer each time, the source unchanged, and the same pixels on both paths"""
    turn = PATS.index(pattern) + FK.FMTS.index(fmt)
    for i, W in enumerate(WIDTHS):
        Hh = HEIGHTS[(i + turn) % len(HEIGHTS)]
        for n in (1, 3):
            for bits in (8, 12):
                p = BC.params(pattern, bits) if (i + n) % 2 else BC.params(pattern, bits, 1 << (bits - 5), (1400, 1024, 1800))
                pixels = []
                for aligned in (True, False):
                    raw = BC.Raw(n, W, Hh, bits, aligned=aligned, seed=W + Hh + bits)
                    dst = FK.pix_layout(n, W, Hh, fmt, aligned, fill=FK.GUARD)
                    want = BC.host_demosaic(L, raw, dst, p)
                    assert (want[~dst.pixel_mask()] == FK.GUARD).all()
                    got, src_after = device_demosaic(oa, det, raw, dst, p)
                    assert (src_after == raw.buf).all()
                    same(got, want, dst.pixel_mask(), "%dx%d x %d %s %d bits -> %s aligned=%s" % (W, Hh, n, pattern, bits, fmt, aligned))
                    pixels.append(np.stack([dst.view(f, got) for f in range(n)]))
                assert (pixels[0] == pixels[1]).all()


@pytest.mark.parametrize("bits", [10, 16])
def test_black_levels_and_gains(oa, L, det, bits):
    """non-default black levels and gains (a gain of 0, the largest gain, black = the largest sample among them) at 10 and 16 bits"""
    for W, Hh in ((17, 6), (513, 5)):
        for k, (black, gains) in enumerate(BC.knobs(bits)):
            pattern, fmt = PATS[k % 4], FK.FMTS[(k + W) % 5]
            p = BC.params(pattern, bits, black, gains)
            for aligned in (True, False):
                raw = BC.Raw(2, W, Hh, bits, aligned=aligned, seed=W + k)
                dst = FK.pix_layout(2, W, Hh, fmt, aligned, fill=FK.GUARD)
                got, src_after = device_demosaic(oa, det, raw, dst, p)
                assert (src_after == raw.buf).all()
                same(got, BC.host_demosaic(L, raw, dst, p), dst.pixel_mask(), "%dx%d %s %d bits black %d gains %s -> %s aligned=%s" % (
                    W, Hh, pattern, bits, black, gains, fmt, aligned))


def test_any_strip_height_gives_the_same_bytes(oa, L):
    """the row pairs a lane marches down are a tuning knob (OCVAR_TUNE_BAYER_PAIRS, 1 .. 64; 0 restores the default): heights either
    side of every strip of 1, 2, 3 and 64 pairs, the host core's buffer each time"""
    det = oa.Detector(64, 32, max_batch=1)
    for pairs, heights in ((1, (2, 3, 5)), (2, (3, 4, 5, 9)), (3, (5, 6, 7, 13)), (64, (17, 127, 128, 129)), (1000, (129,)), (0, (9,))):
        det.set_tuning(bayer_pairs=pairs)
        for k, Hh in enumerate(heights):
            W, bits, fmt, aligned = (17, 521)[k % 2], (8, 12)[(k + pairs) % 2], FK.FMTS[(k + pairs) % 5], bool((k + pairs) % 2)
            p = BC.params(PATS[(k + pairs) % 4], bits, 3, (1100, 1024, 1300))
            raw = BC.Raw(2, W, Hh, bits, aligned=aligned, seed=Hh + pairs)
            dst = FK.pix_layout(2, W, Hh, fmt, aligned, fill=FK.GUARD)
            got, src_after = device_demosaic(oa, det, raw, dst, p)
            assert (src_after == raw.buf).all()
            same(got, BC.host_demosaic(L, raw, dst, p), dst.pixel_mask(), "%d pairs, %dx%d %d bits -> %s aligned=%s" % (pairs, W, Hh, bits, fmt, aligned))


def test_params_none_are_the_defaults(oa, L, det):
    raw = BC.Raw(2, 17, 6, 8, aligned=True, seed=4)
    dst = FK.pix_layout(2, 17, 6, "bgra", True, fill=FK.GUARD)
    got, _ = device_demosaic(oa, det, raw, dst, None)
    same(got, BC.host_demosaic(L, raw, dst, BC.params()), dst.pixel_mask(), "params None")


# ---- chunks and stream order ----------------------------------------------------------------------------------------------------------------

def test_more_frames_than_one_launch_takes(oa, L, det):
    """65537 frames of 2 x 2 samples, stored without a gap: two launches (the grid's z ends at 65535), every frame converted once"""
    import torch
    n, lead = 65537, 64
    rng = np.random.default_rng(2)
    raw = np.full(lead + 4 * n + lead, FK.GUARD, np.uint8)
    raw[lead:lead + 4 * n] = rng.integers(0, 256, 4 * n, dtype=np.uint8)
    pix = np.full(lead + 12 * n + lead, FK.GUARD, np.uint8)
    want = pix.copy()
    p = BC.params("gbrg", 8, 5, (1200, 1024, 1600))
    assert L.bayer_to_frames_emul(raw.ctypes.data + lead, 2, 4, want.ctypes.data + lead, 6, 12, 2, 2, 0, n, C.addressof(p)) == 0
    d, dd = to_device(raw), to_device(pix)
    torch.cuda.synchronize()
    det.bayer_to_frames(d.data_ptr() + lead, dd.data_ptr() + lead, 2, 2, n, params=lib_params(oa, p), fmt="bgr")
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:4].tolist()
    assert (got[lead + 12 * 65535: lead + 12 * n] != FK.GUARD).any()   # (the frames of the second launch)
    assert (d.cpu().numpy() == raw).all()


def test_demosaic_detect_annotate_on_one_stream(oa, L):
    """demosaic -> enqueue -> annotate on the frames behind the batch -> a second demosaic of the same mosaics, all queued on the
    context's stream with nothing waited for before collect: the host cores of every step"""
    import torch
    cfg = H.synth_config(2)   # 640 x 480, four markers
    W, Hh, n = cfg.width, cfg.height, 2
    det, tpls, cam = make_detector(oa, cfg, None, n)
    LA = AC.build_emul()
    st = AC.style(LA, thickness=2)
    raw = BC.Raw(n, W, Hh, 12, aligned=True)
    for f in range(n):
        raw.put(f, BC.mosaic(H.synth_frame(cfg, f)[0], "grbg", 12))
    p = BC.params("grbg", 12)
    bgr, again = FK.pix_layout(n, W, Hh, "bgr", True, fill=FK.GUARD), FK.pix_layout(n, W, Hh, "rgba", False, fill=FK.GUARD)
    want_bgr, want_again = BC.host_demosaic(L, raw, bgr, p), BC.host_demosaic(L, raw, again, p)
    d, db, da = to_device(raw.buf), to_device(bgr.buf), to_device(again.buf)
    torch.cuda.synchronize()
    kw = dict(params=lib_params(oa, p), src_row_stride=raw.row_stride, src_frame_stride=raw.frame_stride)
    det.bayer_to_frames(d.data_ptr() + raw.offset(0), db.data_ptr() + bgr.offset(0), W, Hh, n, fmt="bgr", dst_row_stride=bgr.row_stride,
                        dst_frame_stride=bgr.frame_stride, **kw)
    det.enqueue_device(db.data_ptr() + bgr.offset(0), W, Hh, n, row_stride=bgr.row_stride, frame_stride=bgr.frame_stride)
    det.annotate(db.data_ptr() + bgr.offset(0), W, Hh, style=st, row_stride=bgr.row_stride, frame_stride=bgr.frame_stride)
    det.bayer_to_frames(d.data_ptr() + raw.offset(0), da.data_ptr() + again.offset(0), W, Hh, n, fmt="rgba", dst_row_stride=again.row_stride,
                        dst_frame_stride=again.frame_stride, **kw)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    for f in range(n):
        ref = OracleFrame(np.ascontiguousarray(bgr.view(f, want_bgr)), tpls, cam, planes=False)
        assert len(ref.markers) >= 1
        check_markers(f, ref, markers, counts, where="demosaiced")
    drawn_on, drawn = AC.host_annotate(LA, bgr, markers, counts, st, cam, buf=want_bgr)
    assert min(drawn) >= 1 and (drawn_on != want_bgr).any()
    same(db.cpu().numpy(), drawn_on, bgr.pixel_mask(), "annotated")
    same(da.cpu().numpy(), want_again, again.pixel_mask(), "the second demosaic")
    assert (d.cpu().numpy() == raw.buf).all()


# ---- the chain on the device ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ["640x480", "320x240"])
def test_the_chain_on_the_device(oa, L, size):
    """the mosaiced chain scenes of one size (levels_chain.chain_scenes; frame f in pattern f % 4) demosaiced on the device to BGR
    and to GRAY, each detected: the records of both are byte-identical, and they are the oracle's registration on the host core's
    BGR frames"""
    import torch
    scenes = [bgr for name, bgr in LC.chain_scenes() if name.startswith(size)]
    n, (Hh, W) = len(scenes), scenes[0].shape[:2]
    tpls, cam = H.oracle_templates(), H.oracle_camera(W, Hh)
    det = oa.Detector(W, Hh, max_batch=n)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    bgr, gray = FK.pix_layout(n, W, Hh, "bgr", True, fill=FK.GUARD), FK.pix_layout(n, W, Hh, "gray", False, fill=FK.GUARD)
    db, dg = to_device(bgr.buf), to_device(gray.buf)
    want = bgr.buf.copy()
    for f in range(n):   # (a pattern per frame: a call per frame)
        pattern = PATS[f % 4]
        raw = BC.Raw(1, W, Hh, 8, aligned=True)
        raw.put(0, BC.mosaic(scenes[f], pattern))
        p = BC.params(pattern)
        one = FK.pix_layout(1, W, Hh, "bgr", True, fill=FK.GUARD)
        bgr.view(f, want)[...] = one.view(0, BC.host_demosaic(L, raw, one, p))
        d = to_device(raw.buf)
        torch.cuda.synchronize()
        for dd, lay, fmt in ((db, bgr, "bgr"), (dg, gray, "gray")):
            det.bayer_to_frames(d.data_ptr() + raw.offset(0), dd.data_ptr() + lay.offset(f), W, Hh, 1, params=lib_params(oa, p), fmt=fmt,
                                src_row_stride=raw.row_stride, dst_row_stride=lay.row_stride)
        torch.cuda.synchronize()
    same(db.cpu().numpy(), want, bgr.pixel_mask(), "the BGR frames")
    results = {}
    for dd, lay, fmt in ((db, bgr, "bgr"), (dg, gray, "gray")):
        det.set_input_format(fmt)
        det.enqueue_device(dd.data_ptr() + lay.offset(0), W, Hh, n, row_stride=lay.row_stride, frame_stride=lay.frame_stride)
        m, c = det.collect()
        results[fmt] = (m.copy(), c.copy())
    assert results["bgr"][0].tobytes() == results["gray"][0].tobytes() and (results["bgr"][1] == results["gray"][1]).all()
    for f in range(n):
        ref = OracleFrame(np.ascontiguousarray(bgr.view(f, want)), tpls, cam, planes=False)
        assert len(ref.markers) >= 1
        check_markers(f, ref, *results["bgr"], where=size)


# ---- refusals and the idle context ----------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(64, 32, max_batch=1)
    ctx = det._ctx
    W, Hh, n = 64, 32, 2
    pix_h = np.full(n * 4 * W * Hh + 64, FK.GUARD, np.uint8)
    raw_h = np.full(n * 2 * W * Hh + 64, 77, np.uint8)
    dp, dr = to_device(pix_h), to_device(raw_h)
    torch.cuda.synchronize()
    pp, rp = dp.data_ptr(), dr.data_ptr()
    span = (2 ** 31) // (Hh - 1) + 1       # a stride with which the rows of a frame span more than 2^31 - 1 bytes

    def call(**kw):
        a = dict(src=rp, srs=W, dst=pp, drs=3 * W, w=W, h=Hh, n=n, fmt=0, par=(0, 8, 0, 1024, 1024, 1024))
        a.update(kw)
        par = oa.BayerParams(*a["par"]) if a["par"] is not None else None
        return lib.ocvar_hip_bayer_to_frames(ctx, a["src"], a["srs"], a.get("sfs", a["srs"] * a["h"]), a["dst"], a["drs"], a.get("dfs", a["drs"] * a["h"]),
                                             a["w"], a["h"], a["n"], a["fmt"], C.byref(par) if par is not None else None, None)

    w16 = (0, 12, 0, 1024, 1024, 1024)
    cases = [dict(src=None), dict(dst=None), dict(w=1), dict(h=1), dict(w=0), dict(h=-3), dict(w=32768, srs=32768, drs=3 * 32768), dict(h=32768),
             dict(par=(4, 8, 0, 1024, 1024, 1024)), dict(par=(-1, 8, 0, 1024, 1024, 1024)), dict(fmt=5), dict(fmt=-1),
             dict(par=(0, 7, 0, 1024, 1024, 1024)), dict(par=(0, 17, 0, 1024, 1024, 1024)), dict(par=(0, 8, 256, 1024, 1024, 1024)),
             dict(par=(0, 8, -1, 1024, 1024, 1024)), dict(par=(0, 12, 4096, 1024, 1024, 1024)), dict(par=(0, 8, 0, 16384, 1024, 1024)),
             dict(par=(0, 8, 0, 1024, -1, 1024)), dict(par=(0, 8, 0, 1024, 1024, 16384)),
             dict(srs=W - 1), dict(par=w16, srs=2 * W - 2), dict(drs=3 * W - 1), dict(fmt=2, drs=4 * W - 1), dict(fmt=4, drs=W - 1),
             dict(par=w16, srs=2 * W, src=rp + 1), dict(par=w16, srs=2 * W + 1), dict(par=w16, srs=2 * W, sfs=2 * W * Hh + 1),
             dict(n=0), dict(n=-1), dict(srs=span, sfs=W * Hh, n=1), dict(drs=span, dfs=3 * W * Hh, n=1),
             dict(dst=rp), dict(dst=rp + W * Hh * n - 1), dict(src=pp + 3 * W * Hh * n - 1), dict(src=pp + 5)]
    for kw in cases:
        assert call(**kw) == E_ARG, kw
        text = lib.ocvar_hip_last_error(ctx)
        assert text and text.startswith(b"bayer_to_frames: "), (kw, text)
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == pix_h).all() and (dr.cpu().numpy() == raw_h).all()
    # and after all that the context still converts: with NULL params, and from words at an even address that is no multiple of 4 to GRAY
    assert call(par=None) == 0 and call(par=w16, srs=2 * W, src=rp + 2, dst=pp + 3 * W * Hh * n + 1, drs=W, fmt=4, n=1) == 0
    torch.cuda.synchronize()
    got = dp.cpu().numpy()
    want = pix_h.copy()
    assert L.bayer_to_frames_emul(raw_h.ctypes.data, W, W * Hh, want.ctypes.data, 3 * W, 3 * W * Hh, W, Hh, 0, n, None) == 0
    q = BC.params("rggb", 12)
    assert L.bayer_to_frames_emul(raw_h.ctypes.data + 2, 2 * W, 0, want.ctypes.data + 3 * W * Hh * n + 1, W, 0, W, Hh, 4, 1, C.addressof(q)) == 0
    assert (got == want).all() and (dr.cpu().numpy() == raw_h).all()


def test_the_calls_allocate_nothing(oa):
    """device memory in use is the same before and after the first demosaics of a context that has detected: no workspace.  A
    context of its own makes the first demosaics of the process beforehand (the runtime loads a code object at its first launch).
    The figure is the whole device's, so a difference is looked at again on a fresh context: another process's allocation does not
    repeat, a workspace of these calls would."""
    import torch
    cfg = H.synth_config(2)
    W, Hh, n = cfg.width, cfg.height, 2
    frames = np.stack([H.synth_frame(cfg, f)[0] for f in range(n)])
    d = to_device(frames)
    raw8 = to_device(np.stack([BC.mosaic(frames[f], "rggb") for f in range(n)]))
    raw12 = to_device(np.stack([BC.mosaic(frames[f], "bggr", 12) for f in range(n)]))
    dback = to_device(np.zeros(frames.size, np.uint8))
    dgray = to_device(np.zeros(n * W * Hh, np.uint8))

    def convert(det):
        det.bayer_to_frames(raw8.data_ptr(), dback.data_ptr(), W, Hh, n, fmt="bgr")
        det.bayer_to_frames(raw12.data_ptr(), dgray.data_ptr(), W, Hh, n, params=oa.bayer_params("bggr", 12), fmt="gray")
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
    assert (d.cpu().numpy() == frames.reshape(-1)).all() and dback.cpu().numpy().any() and dgray.cpu().numpy().any()

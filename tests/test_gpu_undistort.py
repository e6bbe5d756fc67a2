"""Undistortion on the device (ocvar_hip_undistort / ocvar_hip_undistort_records) byte for byte against the host build of
undistort_core.h (tests/undistort_chain.py): whole destination buffers are compared, the guard bytes in the row padding, between
the frames and around the block included, and whole record blocks, the slots that are not written included."""
import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import persp_synth as PS
import undistort_chain as UC
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(33, 17), (259, 5), (320, 240)]   # a row that ends inside a lane; a row that crosses the 256-pixel span of a wave; many rows
LENS_NAMES = ["BARREL", "PINCUSHION", "ZERO", "OFF_CENTRE", "WILD"]
SRC_ROW_PAD = 3
N_FRAMES = 3   # on a context of max_batch 2


@pytest.fixture(scope="module")
def L():
    return UC.build_emul()


@pytest.fixture(scope="module")
def det320(oa):
    return oa.Detector(320, 240, max_batch=2)


def set_camera(oa, det, cam):
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))


def dst_layout(W, Hh, fmt, path):
    """the destination of a case: 'dword' -- address, row stride and frame stride multiples of 4 (row padding 4 .. 7 bytes); 'bytes'
    -- a row padding of 1 byte at an odd address"""
    bpp = FK.BPP[FK.FORMATS[fmt]]
    if path == "dword":
        pad = 8 - (W * bpp) % 4 if (W * bpp) % 4 else 4
        d = UC.dst_frames(N_FRAMES, W, Hh, fmt, row_pad=pad, frame_gap=8, lead=FK.LEAD)
        assert d.row_stride % 4 == 0 and d.frame_stride % 4 == 0
    else:
        d = UC.dst_frames(N_FRAMES, W, Hh, fmt, row_pad=1, frame_gap=5, lead=FK.LEAD + 1)
    return d


def device_undistort(det, src, dst, buf=None):
    """det.undistort on device copies of src.buf (or buf) and of the guard-filled dst.buf -> (destination buffer, source buffer
    afterwards)"""
    import torch
    d, dd = to_device(src.buf if buf is None else buf), to_device(dst.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.undistort(d.data_ptr() + src.offset(0), dd.data_ptr() + dst.offset(0), src.width, src.height, src.n, fmt=src.fmt,
                  src_row_stride=src.row_stride, src_frame_stride=src.frame_stride, dst_row_stride=dst.row_stride,
                  dst_frame_stride=dst.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


# every lens with every format; shapes and lane-store paths rotate through them
HAND_MADE = [(fmt, lens, SHAPES[(i + j) % 3], ("dword", "bytes")[(i + j) % 2]) for j, fmt in enumerate(FK.FMTS) for i, lens in enumerate(LENS_NAMES)]


def test_the_hand_made_cases_cover_every_format_with_every_lens_shape_and_store_path():
    for fmt in FK.FMTS:
        mine = [c for c in HAND_MADE if c[0] == fmt]
        assert {c[1] for c in mine} == set(LENS_NAMES) and {c[2] for c in mine} == set(SHAPES) and {c[3] for c in mine} == {"dword", "bytes"}
        for path in ("dword", "bytes"):   # (each path on a row that ends inside a lane, too)
            assert any(c[3] == path and c[2][0] % 4 for c in mine)


@pytest.mark.parametrize("fmt,lens,shape,path", HAND_MADE)
def test_undistort_on_hand_made_shapes(oa, L, det320, fmt, lens, shape, path):
    """three frames on a context of two, a source row padding of 3 bytes; the guard bytes around every destination row and frame
    stay"""
    W, Hh = shape
    cam = UC.camera(W, Hh, lens)
    src = FK.Frames(N_FRAMES, W, Hh, fmt, row_pad=SRC_ROW_PAD, frame_gap=7, seed=W + len(lens))
    dst = dst_layout(W, Hh, fmt, path)
    want = UC.host_undistort(L, src, cam, dst)
    assert (want[~dst.pixel_mask()] == FK.GUARD).all()
    set_camera(oa, det320, cam)
    got, src_after = device_undistort(det320, src, dst)
    assert (src_after == src.buf).all()
    same(got, want, dst, "%dx%d %s %s %s" % (W, Hh, fmt, lens, path))
    if lens == "ZERO":
        for f in range(N_FRAMES):
            assert (dst.view(f, got) == src.view(f)).all()


# ---- records ---------------------------------------------------------------------------------------------------------------------

def lens_records(rng, n, slots, W, Hh):
    """[n, slots] records with every field filled: random squares in and around the frame, the frame's corners, a NaN and a 1e30
    coordinate (an infinite one would make new NaNs, whose sign is the processor's choice)"""
    r = FK.records(rng.uniform(-30, max(W, Hh) + 30, (n * slots, 8)), template_ids=rng.integers(0, 9, n * slots), scores=rng.integers(0, 2, n * slots))
    r["glMatrix"] = rng.normal(size=(n * slots, 16))
    r["aspectRatio"] = rng.uniform(0.5, 2, n * slots)
    r["square"][0] = [0, 0, W - 1, 0, W - 1, Hh - 1, 0, Hh - 1]
    if n * slots >= 4:
        r["square"][1, 3] = np.nan
        r["square"][2, 0] = 1e30
    return r.reshape(n, slots)


@pytest.mark.parametrize("lens", LENS_NAMES)
@pytest.mark.parametrize("slots,in_place", [(1, True), (5, False), (64, True), (64, False)])
def test_undistort_records(oa, L, det320, lens, slots, in_place):
    """counts below, at and above records_per_frame; into the block itself and into another one, whose other slots keep their bytes"""
    import torch
    W, Hh, n = 320, 240, 4
    cam = UC.camera(W, Hh, lens)
    recs = lens_records(np.random.default_rng(slots), n, slots, W, Hh)
    given = [slots - 1, slots, slots + 3, 0]
    want_new = UC.host_records(L, cam, recs, np.minimum(given, slots))
    written = np.arange(slots)[None, :] < np.minimum(given, slots)[:, None]
    before = recs.copy() if in_place else np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, slots).copy()
    want = before.copy()
    want[written] = want_new[written]
    for name in ("glMatrix", "templateId", "markerId", "score", "aspectRatio"):   # (every other field as it was)
        assert want[name][written].tobytes() == recs[name][written].tobytes()
    if lens == "ZERO":
        assert want_new.tobytes() == recs.tobytes()
    elif slots > 1:
        assert (want_new["square"][0, 0] != recs["square"][0, 0]).any()
    set_camera(oa, det320, cam)
    dm, dc = to_device(recs), to_device(np.asarray(given, np.int32))
    do = dm if in_place else to_device(before)
    torch.cuda.synchronize()
    det320.undistort_records(dm.data_ptr(), dc.data_ptr(), n, do.data_ptr(), per_frame=slots)
    torch.cuda.synchronize()
    got = do.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != np.frombuffer(want.tobytes(), np.uint8))[:8].tolist()
    if not in_place:
        assert dm.cpu().numpy().tobytes() == recs.tobytes()


# ---- with detection ----------------------------------------------------------------------------------------------------------------

SCENES = ("ladder-160-0", "ladder-160-2")
PER = 8


@pytest.fixture(scope="module")
def views():
    """the two pinhole scenes, their truly distorted views D under BARREL, and the templates"""
    scenes = [s for s in PS.ladder(lens=False, sizes=(160,)) if s.name in SCENES]
    assert [s.name for s in scenes] == list(SCENES)
    lens_cam = UC.camera(960, 540, "BARREL")
    D = np.stack([UC.distort_image(s.frame, lens_cam) for s in scenes])
    return dict(scenes=scenes, pinhole=scenes[0].cam, lens=lens_cam, D=D, tpls=H.oracle_templates(PS.NAMES))


@pytest.fixture(scope="module")
def det960(oa, views):
    det = oa.Detector(960, 540, max_batch=2)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in views["tpls"]])
    return det


def test_the_camera_travels_by_value(oa, L, det960, views):
    """set_camera(lens), undistort, set_camera(pinhole), enqueue on the undistorted frames, collect -- all on the context's stream,
    nothing waited for in between: the queued undistortion keeps the lens it was called with, the batch gets the pinhole camera"""
    import torch
    v = views
    n, W, Hh = 2, 960, 540
    src, dst = FK.Frames(n, W, Hh, "bgr"), UC.dst_frames(n, W, Hh, "bgr")
    for f in range(n):
        src.view(f)[...] = v["D"][f]
    want = UC.host_undistort(L, src, v["lens"], dst)
    d, dd = to_device(src.buf), to_device(dst.buf)
    torch.cuda.synchronize()
    set_camera(oa, det960, v["lens"])
    det960.undistort(d.data_ptr() + src.offset(0), dd.data_ptr() + dst.offset(0), W, Hh, n)
    set_camera(oa, det960, v["pinhole"])
    det960.enqueue_device(dd.data_ptr() + dst.offset(0), W, Hh, n)
    markers, counts = det960.collect()
    torch.cuda.synchronize()
    same(dd.cpu().numpy(), want, dst, "by value")
    for f in range(n):
        ref = H.oracle_registration(np.ascontiguousarray(dst.view(f, want)), v["tpls"], v["pinhole"])[0]
        assert counts[f] == len(ref) >= 2
        for k, r in enumerate(ref):
            assert (markers[f, k]["square"] == np.array(r.square, np.float32)).all(), (f, k)
            assert markers[f, k]["templateId"] == r.templateId and markers[f, k]["score"] == r.score


def test_records_of_the_distorted_frames(oa, L, det960, views):
    """detection on D with the lens camera, the batch's records copied to a device block, undistort_records on it: the host build's
    result on the device's own records byte for byte, and its squares on the oracle's records of D"""
    import torch
    v = views
    n, W, Hh = 2, 960, 540
    set_camera(oa, det960, v["lens"])
    d = to_device(v["D"])
    dm = to_device(np.full(n * PER * 184, FK.GUARD, np.uint8))
    dc = to_device(np.zeros(n, np.int32))
    do = to_device(np.full(n * PER * 184, FK.GUARD, np.uint8))
    torch.cuda.synchronize()
    det960.enqueue_device(d.data_ptr(), W, Hh, n)
    det960.results_to_device(dm.data_ptr(), dc.data_ptr(), per_frame=PER)
    markers, counts = det960.collect(PER)
    det960.undistort_records(dm.data_ptr(), dc.data_ptr(), n, do.data_ptr(), per_frame=PER)
    torch.cuda.synchronize()
    got = do.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, PER)
    assert (dc.cpu().numpy().view(np.int32) == counts).all() and (counts >= 1).all() and (counts <= PER).all()
    block = dm.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, PER)
    want = np.frombuffer(np.full(n * PER * 184, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, PER).copy()
    mapped = UC.host_records(L, v["lens"], block, counts)
    for f in range(n):
        want[f, :counts[f]] = mapped[f, :counts[f]]
    assert got.tobytes() == want.tobytes()
    for f in range(n):
        ref = H.oracle_registration(v["D"][f], v["tpls"], v["lens"])[0]
        assert counts[f] == len(ref)
        orc = FK.records([list(r.square) for r in ref]).reshape(1, -1)
        sq = UC.host_records(L, v["lens"], orc, [len(ref)])["square"][0]
        assert got["square"][f, :len(ref)].tobytes() == sq.tobytes()
        assert (sq != orc["square"][0]).any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(320, 240, max_batch=2)
    ctx = det._ctx
    W, Hh, M = 320, 240, det.max_markers
    frame = 3 * W * Hh
    d = to_device(np.full(3 * frame, 200, np.uint8))
    out = np.full(2 * frame + 64, FK.GUARD, np.uint8)
    dd = to_device(out)
    recs_h = FK.records([FK.axis_square(5, 5, 50, 50)] * 2).reshape(2, 1)
    recs, cnt = to_device(recs_h), to_device(np.array([1, 1], np.int32))
    ro_h = np.full(2 * 184, FK.GUARD, np.uint8)
    ro = to_device(ro_h)
    torch.cuda.synchronize()
    sp, dp, rp, cp, op = d.data_ptr(), dd.data_ptr(), recs.data_ptr(), cnt.data_ptr(), ro.data_ptr()

    def frames_call(**kw):
        a = dict(sp=sp, srs=3 * W, dp=dp, drs=3 * W, w=W, h=Hh, n=2, fmt=0)
        a.update(kw)
        return lib.ocvar_hip_undistort(ctx, a["sp"], a["srs"], a.get("sfs", a["srs"] * a["h"]), a["dp"], a["drs"], a.get("dfs", a["drs"] * a["h"]),
                                       a["w"], a["h"], a["n"], a["fmt"], None)

    def records_call(**kw):
        a = dict(rp=rp, cp=cp, n=2, per=1, op=op)
        a.update(kw)
        return lib.ocvar_hip_undistort_records(ctx, a["rp"], a["cp"], a["n"], a["per"], a["op"], None)

    def refused(rc, what):
        assert rc == E_ARG, what
        assert lib.ocvar_hip_last_error(ctx), what

    refused(frames_call(), "no camera")
    refused(records_call(), "no camera")
    good = UC.camera(W, Hh, "BARREL")
    for field, index, value in (("cameraMatrix", 0, 0.0), ("cameraMatrix", 4, 0.0), ("cameraMatrix", 0, np.nan), ("cameraMatrix", 4, np.inf),
                                ("cameraMatrix", 2, np.nan), ("cameraMatrix", 5, -np.inf), ("distCoeffs", 0, np.nan), ("distCoeffs", 1, np.inf),
                                ("distCoeffs", 2, np.nan), ("distCoeffs", 3, np.nan), ("distCoeffs", 4, -np.inf)):
        cam = H.Camera.from_buffer_copy(bytes(good))
        getattr(cam, field)[index] = value
        set_camera(oa, det, cam)
        refused(frames_call(), (field, index, value))
        refused(records_call(), (field, index, value))
    set_camera(oa, det, good)
    span = (2 ** 31) // (Hh - 1) + 1   # a row stride with which the rows of one frame span more than 2^31 - 1 bytes
    for kw in [dict(sp=None), dict(dp=None), dict(fmt=5), dict(fmt=-1), dict(srs=3 * W - 1), dict(drs=3 * W - 1), dict(fmt=2, srs=4 * W - 1, drs=4 * W),
               dict(fmt=2, srs=4 * W, drs=4 * W - 1), dict(w=321), dict(h=241), dict(w=0), dict(h=0), dict(n=0), dict(n=-1),
               dict(srs=span, sfs=frame), dict(drs=span, dfs=frame),
               dict(dp=sp), dict(dp=sp + 1), dict(dp=sp + 2 * frame - 1), dict(sp=dp + frame), dict(sp=dp + 2 * frame - 1)]:
        refused(frames_call(**kw), kw)
    for kw in [dict(rp=None), dict(cp=None), dict(op=None), dict(n=0), dict(per=0), dict(per=M + 1)]:
        refused(records_call(**kw), kw)
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == out).all() and (ro.cpu().numpy() == ro_h).all() and (d.cpu().numpy() == 200).all()
    # and after all that the context still undistorts: a destination that ends where the source begins is no overlap
    assert frames_call(sp=sp + frame, dp=sp, n=1) == 0
    assert frames_call() == 0 and records_call() == 0
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got[:2 * frame] == 200).all() and (got[2 * frame:] == FK.GUARD).all()   # (BARREL: nothing outside)
    assert (ro.cpu().numpy().view(FK.MARKER_DTYPE)["templateId"] == 0).all()

"""Resizing on the device (ocvar_hip_resize / ocvar_hip_scale_records) byte for byte against the host build of resize_core.h
(tests/resize_chain.py): whole destination buffers are compared, the guard bytes in the row padding, between the frames and
around the block included, and whole record blocks, the slots that are not written included."""
import itertools

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import overlay_chain as OC
import persp_synth as PS
import resize_chain as RC
from frame_kit import E_ARG, hand_made_records, oa, same, to_device  # noqa: F401
from test_gpu_parity import OracleFrame, check_markers

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4   # tests/test_gpu_parity.py: check_markers


@pytest.fixture(scope="module")
def L():
    return RC.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(64, 32, max_batch=1)   # (neither the sizes nor n_frames are bound by the context's)


def device_resize(det, src, dst, interp, buf=None, src_offset=None, src_size=None):
    """det.resize on device copies of src.buf (or buf) and of dst.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(src.buf if buf is None else buf), to_device(dst.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    sw, sh = (src.width, src.height) if src_size is None else src_size
    torch.cuda.synchronize()
    det.resize(d.data_ptr() + (src.offset(0) if src_offset is None else src_offset), sw, sh, dd.data_ptr() + dst.offset(0), dst.width,
               dst.height, dst.n, interp=interp, fmt=dst.fmt, src_row_stride=src.row_stride, src_frame_stride=src.frame_stride,
               dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------

# the source side of a destination side d: ratio 2, ratio 3, 1.5, below 1, a source of 1; and blocks the two box kernels do not
# take: 4 x 4 and 2 x 3 (the second entry is the height's rule)
RATIOS = [("x2", lambda d: 2 * d, lambda d: 2 * d), ("x3", lambda d: 3 * d, lambda d: 3 * d),
          ("x1.5", lambda d: max(1, 3 * d // 2), lambda d: max(1, 3 * d // 2)), ("x0.67", lambda d: max(1, (2 * d + 2) // 3), lambda d: max(1, (2 * d + 2) // 3)),
          ("one", lambda d: 1, lambda d: 1), ("x4", lambda d: 4 * d, lambda d: 4 * d), ("2x3", lambda d: 2 * d, lambda d: 3 * d)]


@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("interp", list(RC.INTERPS))
def test_resize_sweep(oa, L, det, interp, fmt):
    """every destination width with every ratio, 1 and 3 frames, on the dword path (everything a multiple of 4) and on the byte path
    (an odd lead, odd paddings, a frame gap of 5): the host core's buffer each time, the same pixels on both paths, the source
    untouched; what AREA does not take is refused and nothing written"""
    lib = oa.hip_lib()
    kinds = set()
    for (i, dw), (j, (name, fx, fy)), (k, dh) in itertools.product(enumerate(RC.DST_WIDTHS), enumerate(RATIOS), enumerate(RC.DST_HEIGHTS)):
        sw, sh = fx(dw), fy(dh)
        n = 1 if (i + j + k) % 2 else 3
        where = "%s %s %dx%d -> %dx%d x %d" % (interp, fmt, sw, sh, dw, dh, n)
        pixels = []
        for aligned in (True, False):
            src = FK.pix_layout(n, sw, sh, fmt, aligned, seed=dw + j)
            dst = FK.pix_layout(n, dw, dh, fmt, aligned, fill=FK.GUARD)
            rc, want = RC.host_resize(L, src, dst, interp)
            if interp == "area" and not RC.area_ok(sw, sh, dw, dh):
                assert rc == E_ARG
                d, dd = to_device(src.buf), to_device(dst.buf)
                assert lib.ocvar_hip_resize(det._ctx, d.data_ptr() + src.offset(0), sw, sh, src.row_stride, src.frame_stride,
                                            dd.data_ptr() + dst.offset(0), dw, dh, dst.row_stride, dst.frame_stride, n, dst.fmt, 2, None) == E_ARG, where
                assert lib.ocvar_hip_last_error(det._ctx)
                assert (dd.cpu().numpy() == dst.buf).all()
                continue
            assert rc == 0 and (want[~dst.pixel_mask()] == FK.GUARD).all()
            got, src_after = device_resize(det, src, dst, interp)
            assert (src_after == src.buf).all(), where
            same(got, want, dst.pixel_mask(), where + " aligned=%s" % aligned)
            pixels.append(np.stack([dst.view(f, got) for f in range(n)]))
            plan = np.zeros(3, np.int32)
            L.resize_plan_emul(sw, sh, dw, dh, RC.INTERPS[interp], H.P(plan))
            kinds.add((int(plan[0]), int(plan[1]), int(plan[2])) if plan[0] == RC.KIND_BOX else int(plan[0]))
        if pixels:
            assert (pixels[0] == pixels[1]).all(), where
    # every kernel the mode has was run: the gathering one, and for the boxes both box kernels and the gathering one
    boxes = {(RC.KIND_BOX, 2, 2), (RC.KIND_BOX, 3, 3), (RC.KIND_BOX, 4, 4), (RC.KIND_BOX, 2, 3), (RC.KIND_BOX, 1, 1)}
    assert kinds == {"nearest": {0}, "linear": {1, (RC.KIND_BOX, 2, 2)}, "area": boxes | {RC.KIND_TABLE}}[interp], kinds


def test_a_box_source_that_is_unaligned_under_an_aligned_destination(oa, L, det):
    """the box kernels load whole dwords only when the source is aligned too"""
    for k in (2, 3):
        src = FK.pix_layout(2, k * 37, k * 3, "bgr", False, seed=k)
        dst = FK.pix_layout(2, 37, 3, "bgr", True, fill=FK.GUARD)
        rc, want = RC.host_resize(L, src, dst, "area")
        got, _ = device_resize(det, src, dst, "area")
        same(got, want, dst.pixel_mask(), "box %d" % k)


def test_the_largest_ratio_of_the_table(oa, L, det):
    """AREA at a ratio just below 16 on both axes: 18 x 18 taps at most"""
    src = FK.pix_layout(1, 16 * 21 - 5, 16 * 3 - 1, "bgra", True, seed=3)
    dst = FK.pix_layout(1, 21, 3, "bgra", True, fill=FK.GUARD)
    rc, want = RC.host_resize(L, src, dst, "area")
    assert rc == 0
    got, _ = device_resize(det, src, dst, "area")
    same(got, want, dst.pixel_mask(), "ratio 16")


# ---- a source rectangle ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interp", list(RC.INTERPS))
@pytest.mark.parametrize("aligned", [True, False])
def test_source_rectangle(oa, L, det, interp, aligned):
    """a rectangle inside a larger guarded frame, as a pointer offset with the full frame's strides: the bytes of the cropped copy"""
    n, fmt = 2, "bgr"
    big = FK.pix_layout(n, 150, 40, fmt, aligned, seed=11)
    x0, y0, rw, rh = (8 if aligned else 7), 5, 96, 30     # (8 pixels of 3 bytes keep the aligned case aligned)
    dw, dh = 48, 15
    off = big.offset(0) + y0 * big.row_stride + x0 * big.bpp
    crop = FK.pix_layout(n, rw, rh, fmt, aligned)
    for f in range(n):
        crop.view(f)[...] = big.view(f)[y0:y0 + rh, x0:x0 + rw]
    dst = FK.pix_layout(n, dw, dh, fmt, aligned, fill=FK.GUARD)
    rc, want_crop = RC.host_resize(L, crop, dst, interp)
    rc2, want = RC.host_resize(L, big, dst, interp, src_offset=off, src_size=(rw, rh))
    assert rc == 0 and rc2 == 0 and (want == want_crop).all()
    got, src_after = device_resize(det, big, dst, interp, src_offset=off, src_size=(rw, rh))
    assert (src_after == big.buf).all()
    same(got, want, dst.pixel_mask(), "rectangle %s aligned=%s" % (interp, aligned))


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------

def test_more_frames_than_one_launch_takes(oa, L, det):
    """65537 frames of 2 x 2 pixels to 1 x 1, stored without a gap: two launches (the grid's z ends at 65535), every frame once"""
    import torch
    n, lead = 65537, 64
    rng = np.random.default_rng(2)
    src = np.full(lead + 12 * n + lead, FK.GUARD, np.uint8)
    src[lead:lead + 12 * n] = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    dst = np.full(lead + 3 * n + lead, FK.GUARD, np.uint8)
    want = dst.copy()
    assert L.resize_emul(src.ctypes.data + lead, 2, 2, 6, 12, want.ctypes.data + lead, 1, 1, 3, 3, n, 0, 2) == 0
    d, dd = to_device(src), to_device(dst)
    torch.cuda.synchronize()
    det.resize(d.data_ptr() + lead, 2, 2, dd.data_ptr() + lead, 1, 1, n, interp="area", fmt="bgr")
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:4].tolist()
    assert (got[lead + 3 * 65535: lead + 3 * n] != FK.GUARD).any()   # (the frames of the second launch)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(32, 16, max_batch=1)
    ctx = det._ctx
    SW, SH, DW, DH, n = 64, 32, 32, 16, 2
    src_h = np.full(n * 4 * SW * SH + 64, 77, np.uint8)
    dst_h = np.full(n * 4 * SW * SH + 64, FK.GUARD, np.uint8)
    ds, dd = to_device(src_h), to_device(dst_h)
    torch.cuda.synchronize()
    sp, dp = ds.data_ptr(), dd.data_ptr()
    span = (2 ** 31) // (SH - 1) + 1      # a row stride with which the rows of the source span more than 2^31 - 1 bytes
    span_d = (2 ** 31) // (DH - 1) + 1

    def call(**kw):
        a = dict(src=sp, sw=SW, sh=SH, srs=3 * SW, dst=dp, dw=DW, dh=DH, drs=3 * DW, n=n, fmt=0, interp=2)
        a.update(kw)
        return lib.ocvar_hip_resize(ctx, a["src"], a["sw"], a["sh"], a["srs"], a.get("sfs", a["srs"] * a["sh"]), a["dst"], a["dw"], a["dh"],
                                    a["drs"], a.get("dfs", a["drs"] * a["dh"]), a["n"], a["fmt"], a["interp"], None)

    cases = [dict(src=None), dict(dst=None), dict(fmt=5), dict(fmt=-1), dict(interp=3), dict(interp=-1),
             dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(sw=-1), dict(sw=32768, srs=3 * 32768, interp=0), dict(sh=32768, interp=0),
             dict(dw=32768, drs=3 * 32768, interp=0), dict(dh=32768, interp=0),
             dict(srs=3 * SW - 1), dict(drs=3 * DW - 1), dict(fmt=2, srs=4 * SW - 1), dict(fmt=2, srs=4 * SW, drs=4 * DW - 1), dict(fmt=4, srs=SW, drs=DW - 1),
             dict(srs=span, sfs=3 * SW * SH, n=1), dict(drs=span_d, dfs=3 * DW * DH, n=1),
             dict(n=0), dict(n=-1),
             dict(dst=sp), dict(dst=sp + 3 * SW * SH * n - 1), dict(src=dp + 3 * DW * DH * n - 1), dict(src=dp + 1),
             dict(dw=SW + 1, drs=3 * (SW + 1)), dict(dh=SH + 1), dict(sw=16 * DW + 1, srs=3 * (16 * DW + 1)), dict(sh=16 * DH + 1)]
    for rounds in range(2):
        for kw in cases:
            assert call(**kw) == E_ARG, kw
            assert lib.ocvar_hip_last_error(ctx), kw
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == dst_h).all() and (ds.cpu().numpy() == src_h).all()
    with pytest.raises(ValueError):
        det.resize(sp, SW, SH, dp, DW, DH, n, interp="cubic")
    with pytest.raises(ValueError):
        det.resize(sp, SW, SH, dp, DW, DH, n, interp=2)
    # after all that the context still resizes; a source larger than the context's maximum all along
    assert call() == 0
    torch.cuda.synchronize()
    want = dst_h.copy()
    assert L.resize_emul(src_h.ctypes.data, SW, SH, 3 * SW, 3 * SW * SH, want.ctypes.data, DW, DH, 3 * DW, 3 * DW * DH, n, 0, 2) == 0
    assert (dd.cpu().numpy() == want).all()
    # what the other modes take of AREA's refusals: enlarging, and any ratio
    assert call(dw=SW + 1, drs=3 * (SW + 1), interp=1) == 0 and call(sw=16 * DW + 1, sh=4, srs=3 * (16 * DW + 1), interp=0, n=1) == 0
    torch.cuda.synchronize()

    # scale_records
    recs = to_device(np.zeros(2 * 4, FK.MARKER_DTYPE))
    counts = to_device(np.array([4, 4], np.int32))
    before = recs.cpu().numpy().copy()

    def rcall(**kw):
        a = dict(m=recs.data_ptr(), c=counts.data_ptr(), n=2, per=4, sw=DW, sh=DH, dw=SW, dh=SH, flags=0, out=recs.data_ptr())
        a.update(kw)
        return lib.ocvar_hip_scale_records(ctx, a["m"], a["c"], a["n"], a["per"], a["sw"], a["sh"], a["dw"], a["dh"], a["flags"], a["out"], None)

    rcases = [dict(m=None), dict(c=None), dict(out=None), dict(n=0), dict(n=-1), dict(per=0), dict(per=det.max_markers + 1),
              dict(sw=0), dict(sh=32768), dict(dw=0), dict(dh=-3), dict(flags=2), dict(flags=-1), dict(flags=1)]   # (flags=1: no camera is set)
    for kw in rcases:
        assert rcall(**kw) == E_ARG, kw
        assert lib.ocvar_hip_last_error(ctx), kw
    torch.cuda.synchronize()
    assert (recs.cpu().numpy() == before).all()
    assert rcall() == 0
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(SW, SH))))
    assert rcall(flags=1) == 0
    torch.cuda.synchronize()


# ---- scale_records --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("slots,in_place", [(1, True), (5, False), ("all", True), ("all", False)])
def test_scale_records(oa, L, dense, pose, slots, in_place):
    """counts of 0, 1, per_frame and more; into the block itself and into another one, whose other slots keep their guard bytes;
    every field but the square (and glMatrix with the pose flag) bit for bit as it was, the square the host core's bits, glMatrix
    the host pose core's on the new square within check_markers' tolerance"""
    import torch
    small, large = (640, 480), (1920, 1080)   # (the two axes scale differently: 3 and 2.25)
    det = oa.Detector(64, 32, max_batch=1, max_markers=200) if dense else oa.Detector(64, 32, max_batch=1)
    slots = det.max_markers if slots == "all" else slots
    n = 4
    cam = H.oracle_camera(*large)
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    recs = hand_made_records(np.random.default_rng(slots + dense), n, slots, *small)
    if not pose and slots >= 4:
        recs["square"][0, 1, 3] = np.nan
        recs["square"][0, 2, 0] = 1e30
    given = [0, 1, slots, slots + 3]
    live = np.minimum(given, slots)
    want_new = RC.host_scale_records(L, recs, live, small, large, pose=pose, cam=cam)
    written = np.arange(slots)[None, :] < live[:, None]
    guard = np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, slots)
    before = recs.copy() if in_place else guard.copy()
    want = before.copy()
    want[written] = want_new[written]
    assert want_new["square"][written].view(np.uint32).tolist() == RC.np_scale_squares(recs["square"], small, large)[written].view(np.uint32).tolist()
    assert (want_new["glMatrix"][written] != recs["glMatrix"][written]).any() == pose
    dm, dc = to_device(recs), to_device(np.asarray(given, np.int32))
    do = dm if in_place else to_device(before)
    torch.cuda.synchronize()
    det.scale_records(dm.data_ptr(), dc.data_ptr(), n, do.data_ptr(), small, large, per_frame=slots, pose=pose)
    torch.cuda.synchronize()
    got = do.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, slots)
    if pose:
        g, w = got["glMatrix"][written], want["glMatrix"][written]
        for a, b in zip(g, w):
            assert np.abs(a - b).max() <= POSE_RTOL * max(1.0, np.abs(b).max()), (a, b)
        got = got.copy()
        got["glMatrix"][written] = want["glMatrix"][written]
    assert got.tobytes() == want.tobytes(), np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))[:8].tolist()
    if not in_place:
        assert dm.cpu().numpy().tobytes() == recs.tobytes()


def test_scale_records_takes_the_camera_of_the_call(oa, L):
    """OCVAR_SCALE_POSE with camera A, set_camera(B) right after the call, nothing waited for: the poses are camera A's"""
    import torch
    small, large = (640, 480), (1280, 960)
    det = oa.Detector(64, 32, max_batch=1)
    cam_a, cam_b = H.oracle_camera(*large), PS.camera(*large, wide=1.5)
    recs = hand_made_records(np.random.default_rng(4), 1, 6, *small)
    want_a = RC.host_scale_records(L, recs, [6], small, large, pose=True, cam=cam_a)
    want_b = RC.host_scale_records(L, recs, [6], small, large, pose=True, cam=cam_b)
    assert np.abs(want_a["glMatrix"] - want_b["glMatrix"]).max() > 1e-2
    dm, dc = to_device(recs), to_device(np.array([6], np.int32))
    torch.cuda.synchronize()
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam_a)))
    det.scale_records(dm.data_ptr(), dc.data_ptr(), 1, dm.data_ptr(), small, large, per_frame=6, pose=True)
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam_b)))
    torch.cuda.synchronize()
    got = dm.cpu().numpy().view(FK.MARKER_DTYPE).reshape(1, 6)
    for a, b in zip(got["glMatrix"][0], want_a["glMatrix"][0]):
        assert np.abs(a - b).max() <= POSE_RTOL * max(1.0, np.abs(b).max())
    assert got["square"].tobytes() == want_a["square"].tobytes()


# ---- the chain on the device ------------------------------------------------------------------------------------------------------------

COLOUR = np.array([250, 10, 200, 255], np.uint8)   # R G B A


def test_the_chain_on_the_device(oa, L):
    """the feature end to end: the CPU chain's 1280 x 960 scenes shrunk by 2 on the device (AREA), detected by a 640 x 480 context
    with the camera of that size, the records handed over on the device, scaled up with the pose of the large camera and drawn on
    the large frames -- the oracle's markers on the host core's small frames, the host core's scaled records bit for bit, the
    host rendering under those records byte for byte"""
    import torch
    (W, Hh), (FW, FH) = RC.CHAIN_SMALL, RC.CHAIN_FULL
    scenes = RC.chain_scenes()
    n = len(scenes)
    tpls = RC.chain_templates()
    cam_small, cam_full = PS.camera(W, Hh), PS.camera(FW, FH)
    det = oa.Detector(W, Hh, max_batch=n)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam_small)))
    painter = oa.Detector(FW, FH, max_batch=1)     # render_records is bound by its context's size: a context for drawing
    overlay = np.broadcast_to(COLOUR, (4, 4, 4)).copy()
    painter.set_overlay(-1, overlay)
    painter.set_camera(oa.Camera.from_buffer_copy(bytes(cam_full)))
    full = FK.pix_layout(n, FW, FH, "bgr", True)
    for f, sc in enumerate(scenes):
        full.view(f)[...] = sc.frame
    small = FK.pix_layout(n, W, Hh, "bgr", True, fill=FK.GUARD)
    rc, want_small = RC.host_resize(L, full, small, "area")
    assert rc == 0
    M = det.max_markers
    d_full, d_small = to_device(full.buf), to_device(small.buf)
    d_recs, d_counts = to_device(np.full(n * M * FK.MARKER_DTYPE.itemsize, FK.GUARD, np.uint8)), to_device(np.zeros(n, np.int32))
    d_up = to_device(np.full(n * M * FK.MARKER_DTYPE.itemsize, FK.GUARD, np.uint8))
    torch.cuda.synchronize()
    # one stream, nothing waited for in between
    s = det.stream_ptr()
    det.resize(d_full.data_ptr() + full.offset(0), FW, FH, d_small.data_ptr() + small.offset(0), W, Hh, n, interp="area", fmt="bgr",
               src_row_stride=full.row_stride, src_frame_stride=full.frame_stride, dst_row_stride=small.row_stride,
               dst_frame_stride=small.frame_stride)
    det.enqueue_device(d_small.data_ptr() + small.offset(0), W, Hh, n, row_stride=small.row_stride, frame_stride=small.frame_stride)
    det.results_to_device(d_recs.data_ptr(), d_counts.data_ptr())
    painter.scale_records(d_recs.data_ptr(), d_counts.data_ptr(), n, d_up.data_ptr(), (W, Hh), (FW, FH), per_frame=M, pose=True, stream=s)
    painter.render_records(d_full.data_ptr() + full.offset(0), FW, FH, n, d_up.data_ptr(), d_counts.data_ptr(), per_frame=M, fmt="bgr",
                           row_stride=full.row_stride, frame_stride=full.frame_stride, stream=s)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    same(d_small.cpu().numpy(), want_small, small.pixel_mask(), "the shrunk frames")
    for f in range(n):
        ref = OracleFrame(np.ascontiguousarray(small.view(f, want_small)), tpls, cam_small, planes=False)
        assert len(ref.markers) == 1
        check_markers(f, ref, markers, counts, where="chain")
    recs = d_recs.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, M)
    assert all(recs[f, :counts[f]].tobytes() == markers[f, :counts[f]].tobytes() for f in range(n))
    want_up = RC.host_scale_records(L, recs, counts, (W, Hh), (FW, FH), pose=True, cam=cam_full)
    got_up = d_up.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, M).copy()
    for f in range(n):
        for k in range(counts[f]):
            a, b = got_up[f, k]["glMatrix"], want_up[f, k]["glMatrix"]
            assert np.abs(a - b).max() <= POSE_RTOL * max(1.0, np.abs(b).max())
            got_up[f, k]["glMatrix"] = b
            m, kk, d = PS.match(got_up[f, k]["square"], scenes[f].markers)
            assert m is scenes[f].markers[0] and kk is not None, (f, d)
    want_guarded = np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, M).copy()
    for f in range(n):
        want_guarded[f, :counts[f]] = want_up[f, :counts[f]]
    assert got_up.tobytes() == want_guarded.tobytes()
    LO = OC.build_emul()
    rendered, drawn = OC.host_render(LO, full, want_guarded, counts, {-1: overlay})
    assert min(drawn) >= 1 and (rendered != full.buf).any()
    same(d_full.cpu().numpy(), rendered, full.pixel_mask(), "rendered")

"""Turning and mirroring on the device (ocvar_hip_orient / ocvar_hip_orient_records) byte for byte against the host build of
orient_core.h (tests/orient_chain.py): whole destination buffers are compared, the guard bytes in the row padding, between the
frames and around the block included, and whole record blocks, the slots that are not written included."""
import itertools

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import orient_chain as OR
import overlay_chain as OC
import persp_synth as PS
from frame_kit import E_ARG, hand_made_records, oa, same, to_device  # noqa: F401
from test_gpu_parity import OracleFrame, check_markers

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4   # tests/test_gpu_parity.py: check_markers
# widths and heights that straddle the transposing kernel's run (4), the row kernels' run (8), the tile (64), two tiles; the widths
# also a wave's span of the row kernels (512)
WIDTHS = [1, OR.TILE_RUN + 1, OR.LANE_PX - 1, OR.LANE_PX + 1, OR.TILE - 1, OR.TILE + 1, 2 * OR.TILE + 1, OR.WAVE_PX + 1]
HEIGHTS = [1, OR.ROW_GROUP + 1, 2 * OR.ROW_GROUP, OR.TILE, OR.TILE + 1, 2 * OR.TILE + 2]     # (and the row kernels' group of 4 rows)


@pytest.fixture(scope="module")
def L():
    return OR.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(64, 32, max_batch=1)   # (neither the sizes nor n_frames are bound by the context's)


def device_orient(det, src, dst, o, buf=None, src_offset=None, src_size=None):
    """det.orient on device copies of src.buf (or buf) and of dst.buf -> (destination buffer, source buffer afterwards)"""
    import torch
    d, dd = to_device(src.buf if buf is None else buf), to_device(dst.buf)
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    sw, sh = (src.width, src.height) if src_size is None else src_size
    torch.cuda.synchronize()
    det.orient(d.data_ptr() + (src.offset(0) if src_offset is None else src_offset), sw, sh, dd.data_ptr() + dst.offset(0), dst.n, o, fmt=dst.fmt,
               src_row_stride=src.row_stride, src_frame_stride=src.frame_stride, dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), d.cpu().numpy()


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
def test_orient_sweep(oa, L, det, fmt):
    """every orientation on every width x height, 1 and 3 frames, on the dword path (everything a multiple of 4) and on the byte path
    (an odd lead, odd paddings, a frame gap of 5): the host core's buffer each time, the same pixels on both paths, the source
    untouched; each of the three kernel classes was run"""
    classes = set()
    for (i, w), (k, h), o in itertools.product(enumerate(WIDTHS), enumerate(HEIGHTS), range(8)):
        n = 1 if (i + k + o) % 2 else 3
        where = "%s %s %dx%d x %d" % (OR.NAMES[o], fmt, w, h, n)
        pixels = []
        for aligned in (True, False):
            src = FK.pix_layout(n, w, h, fmt, aligned, seed=w + k)
            dst = OR.dst_layout(src, o, aligned)
            rc, want = OR.host_orient(L, src, dst, o)
            assert rc == 0 and (want[~dst.pixel_mask()] == FK.GUARD).all()
            got, src_after = device_orient(det, src, dst, o)
            assert (src_after == src.buf).all(), where
            same(got, want, dst.pixel_mask(), where + " aligned=%s" % aligned)
            pixels.append(np.stack([dst.view(f, got) for f in range(n)]))
        assert (pixels[0] == pixels[1]).all(), where
        classes.add(OR.CLASS[o])
    assert classes == {"rows kept", "rows reversed", "transposing"}


def test_reversed_rows_whose_width_is_no_multiple_of_four(oa, L, det):
    """the row-reversing kernels load whole dwords only when the bytes of a row are a multiple of 4: aligned frames of 1 and 3 bytes
    per pixel whose rows are not, next to ones whose rows are"""
    for fmt, w in [("gray", 30), ("gray", 32), ("gray", 521), ("bgr", 30), ("bgr", 32), ("bgr", 523)]:
        for o in ("flip_h", "rot180"):
            src = FK.pix_layout(2, w, 3, fmt, True, seed=w)
            dst = OR.dst_layout(src, o, True)
            rc, want = OR.host_orient(L, src, dst, o)
            got, _ = device_orient(det, src, dst, o)
            same(got, want, dst.pixel_mask(), "%s %s %d" % (o, fmt, w))


# ---- a source rectangle ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False])
def test_source_rectangle(oa, L, det, aligned):
    """a rectangle inside a larger guarded frame, as a pointer offset with the full frame's strides, into a padded destination: the
    bytes of the cropped copy, for every orientation"""
    n, fmt = 2, "bgr"
    big = FK.pix_layout(n, 150, 90, fmt, aligned, seed=11)
    x0, y0, rw, rh = (8 if aligned else 7), 5, 96, 70     # (8 pixels of 3 bytes keep the aligned case aligned)
    off = big.offset(0) + y0 * big.row_stride + x0 * big.bpp
    crop = FK.pix_layout(n, rw, rh, fmt, aligned)
    for f in range(n):
        crop.view(f)[...] = big.view(f)[y0:y0 + rh, x0:x0 + rw]
    for o in range(8):
        dst = OR.dst_layout(crop, o, aligned)
        rc, want_crop = OR.host_orient(L, crop, dst, o)
        rc2, want = OR.host_orient(L, big, dst, o, src_offset=off, src_size=(rw, rh))
        assert rc == 0 and rc2 == 0 and (want == want_crop).all()
        got, src_after = device_orient(det, big, dst, o, src_offset=off, src_size=(rw, rh))
        assert (src_after == big.buf).all()
        same(got, want, dst.pixel_mask(), "rectangle %s aligned=%s" % (OR.NAMES[o], aligned))


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------

def test_more_frames_than_one_launch_takes(oa, L, det):
    """65537 frames of 2 x 1 GRAY pixels under ROT90_CW, stored without a gap: two launches (the grid's z ends at 65535), every frame
    once"""
    import torch
    n, lead = 65537, 64
    rng = np.random.default_rng(2)
    src = np.full(lead + 2 * n + lead, FK.GUARD, np.uint8)
    src[lead:lead + 2 * n] = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    dst = np.full(lead + 2 * n + lead, FK.GUARD, np.uint8)
    want = dst.copy()
    assert L.orient_emul(src.ctypes.data + lead, 2, 1, 2, 2, want.ctypes.data + lead, 1, 2, n, FK.FORMATS["gray"], 1) == 0
    assert (want[lead:lead + 2 * n] == src[lead:lead + 2 * n]).all()    # (a 2 x 1 row turned clockwise is the same two bytes as a column)
    d, dd = to_device(src), to_device(dst)
    torch.cuda.synchronize()
    det.orient(d.data_ptr() + lead, 2, 1, dd.data_ptr() + lead, n, "rot90", fmt="gray")
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:4].tolist()
    assert (got[lead + 2 * 65535: lead + 2 * n] != FK.GUARD).any()   # (the frames of the second launch)
    # and under ROT270_CW every frame's two bytes are swapped
    dd = to_device(dst)
    det.orient(d.data_ptr() + lead, 2, 1, dd.data_ptr() + lead, n, "rot270", fmt="gray")
    torch.cuda.synchronize()
    assert (dd.cpu().numpy()[lead:lead + 2 * n].reshape(n, 2) == src[lead:lead + 2 * n].reshape(n, 2)[:, ::-1]).all()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(32, 16, max_batch=1)
    ctx = det._ctx
    SW, SH, n = 64, 32, 2
    src_h = np.full(n * 4 * SW * SH + 64, 77, np.uint8)
    dst_h = np.full(n * 4 * SW * SH + 64, FK.GUARD, np.uint8)
    ds, dd = to_device(src_h), to_device(dst_h)
    torch.cuda.synchronize()
    sp, dp = ds.data_ptr(), dd.data_ptr()
    span = (2 ** 31) // (SH - 1) + 1      # a row stride with which the rows of the source span more than 2^31 - 1 bytes
    span_t = (2 ** 31) // (SW - 1) + 1    # the same for a transposed destination (SW rows)

    def call(**kw):
        a = dict(src=sp, sw=SW, sh=SH, srs=3 * SW, dst=dp, n=n, fmt=0, o=0)
        a.update(kw)
        dw, dh = OR.oriented_size((a["sw"], a["sh"]), a["o"]) if 0 <= a["o"] < 8 else (a["sw"], a["sh"])
        drs = a.get("drs", 3 * max(dw, 1))
        return lib.ocvar_hip_orient(ctx, a["src"], a["sw"], a["sh"], a["srs"], a.get("sfs", a["srs"] * max(a["sh"], 1)), a["dst"], drs,
                                    a.get("dfs", drs * max(dh, 1)), a["n"], a["fmt"], a["o"], None)

    cases = [dict(src=None), dict(dst=None), dict(fmt=5), dict(fmt=-1), dict(o=8), dict(o=-1),
             dict(sw=0), dict(sh=0), dict(sw=-1), dict(sw=32768, srs=3 * 32768), dict(sh=32768), dict(sh=32768, o=1),
             dict(srs=3 * SW - 1), dict(drs=3 * SW - 1), dict(o=1, drs=3 * SH - 1), dict(o=6, drs=3 * SH - 1),
             dict(fmt=2, srs=4 * SW - 1), dict(fmt=2, srs=4 * SW, drs=4 * SW - 1), dict(fmt=4, srs=SW, drs=SW - 1, o=4),
             dict(srs=span, sfs=3 * SW * SH, n=1), dict(drs=span, dfs=3 * SW * SH, n=1), dict(o=3, drs=span_t, dfs=3 * SW * SH, n=1),
             dict(n=0), dict(n=-1),
             dict(dst=sp), dict(dst=sp, o=2), dict(dst=sp + 3 * SW * SH * n - 1), dict(src=dp + 3 * SW * SH * n - 1, o=1), dict(src=dp + 1, o=7)]
    for rounds in range(2):
        for kw in cases:
            assert call(**kw) == E_ARG, kw
            assert lib.ocvar_hip_last_error(ctx), kw
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == dst_h).all() and (ds.cpu().numpy() == src_h).all()
    with pytest.raises(ValueError):
        det.orient(sp, SW, SH, dp, n, "rot45")
    with pytest.raises(ValueError):
        det.orient(sp, SW, SH, dp, n, 8)
    # after all that the context still turns frames; a source larger than the context's maximum all along
    for o in (0, 1):
        assert call(o=o) == 0
        torch.cuda.synchronize()
        dw, dh = OR.oriented_size((SW, SH), o)
        want = dst_h.copy()
        assert L.orient_emul(src_h.ctypes.data, SW, SH, 3 * SW, 3 * SW * SH, want.ctypes.data, 3 * dw, 3 * dw * dh, n, 0, o) == 0
        assert (dd.cpu().numpy() == want).all()

    # orient_records
    recs = to_device(np.zeros(2 * 4, FK.MARKER_DTYPE))
    counts = to_device(np.array([4, 4], np.int32))
    before = recs.cpu().numpy().copy()

    def rcall(**kw):
        a = dict(m=recs.data_ptr(), c=counts.data_ptr(), n=2, per=4, sw=SW, sh=SH, o=1, flags=0, out=recs.data_ptr())
        a.update(kw)
        return lib.ocvar_hip_orient_records(ctx, a["m"], a["c"], a["n"], a["per"], a["sw"], a["sh"], a["o"], a["flags"], a["out"], None)

    rcases = [dict(m=None), dict(c=None), dict(out=None), dict(n=0), dict(n=-1), dict(per=0), dict(per=det.max_markers + 1),
              dict(sw=0), dict(sh=32768), dict(sw=-3), dict(o=8), dict(o=-1), dict(flags=2), dict(flags=-1), dict(flags=1)]   # (flags=1: no camera is set)
    for kw in rcases:
        assert rcall(**kw) == E_ARG, kw
        assert lib.ocvar_hip_last_error(ctx), kw
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(SH, SW))))
    for o in OR.MIRRORING:     # a reflected view has no rigid pose
        assert rcall(o=o, flags=1) == E_ARG and lib.ocvar_hip_last_error(ctx)
        with pytest.raises(oa.OcvarError):
            det.orient_records(recs.data_ptr(), counts.data_ptr(), 2, recs.data_ptr(), (SW, SH), o, per_frame=4, pose=True)
    torch.cuda.synchronize()
    assert (recs.cpu().numpy() == before).all()
    assert rcall() == 0 and rcall(flags=1) == 0 and rcall(o=4) == 0
    torch.cuda.synchronize()
    # the host-only camera call
    cam, out = H.oracle_camera(SW, SH), H.Camera()
    import ctypes as C
    assert lib.ocvar_hip_orient_camera(None, 1, C.byref(out)) == E_ARG and lib.ocvar_hip_orient_camera(C.byref(cam), 1, None) == E_ARG
    assert lib.ocvar_hip_orient_camera(C.byref(cam), 8, C.byref(out)) == E_ARG
    assert lib.ocvar_hip_orient_camera(C.byref(cam), 1, C.byref(out)) == 0 and bytes(out) == bytes(OR.host_orient_camera(L, cam, 1)[1])


# ---- orient_records -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("slots,in_place", [(1, True), (5, False), ("all", True), ("all", False)])
def test_orient_records(oa, L, pose, slots, in_place):
    """every orientation (with the pose flag: the four rotations); counts of 0, 1, per_frame and more; into the block itself and into
    another one, whose other slots keep their guard bytes; every field but the square (and glMatrix with the pose flag) bit for bit
    as it was, the square the host core's bits, glMatrix the host pose core's on the new square within check_markers' tolerance"""
    import torch
    size = (640, 480)
    det = oa.Detector(64, 32, max_batch=1)
    slots = det.max_markers if slots == "all" else slots
    n = 4
    cam = PS.camera(*size, lens=True)
    for o in (OR.ROTATIONS if pose else range(8)):
        rc, cam_o = OR.host_orient_camera(L, cam, o)
        det.set_camera(oa.orient_camera(oa.Camera.from_buffer_copy(bytes(cam)), o))
        recs = hand_made_records(np.random.default_rng(slots + o), n, slots, *size)
        if not pose and slots >= 4:
            recs["square"][0, 1, 3] = np.nan
            recs["square"][0, 2, 0] = 1e30
        given = [0, 1, slots, slots + 3]
        live = np.minimum(given, slots)
        rc, want_new = OR.host_orient_records(L, recs, live, size, o, pose=pose, cam=cam_o)
        assert rc == 0
        written = np.arange(slots)[None, :] < live[:, None]
        guard = np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, slots)
        before = recs.copy() if in_place else guard.copy()
        want = before.copy()
        want[written] = want_new[written]
        assert want_new["square"][written].view(np.uint32).tolist() == OR.np_orient_squares(recs["square"], size, o)[written].view(np.uint32).tolist()
        dm, dc = to_device(recs), to_device(np.asarray(given, np.int32))
        do = dm if in_place else to_device(before)
        torch.cuda.synchronize()
        det.orient_records(dm.data_ptr(), dc.data_ptr(), n, do.data_ptr(), size, o, per_frame=slots, pose=pose)
        torch.cuda.synchronize()
        got = do.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, slots)
        if pose:
            g, w = got["glMatrix"][written], want["glMatrix"][written]
            for a, b in zip(g, w):
                assert np.abs(a - b).max() <= POSE_RTOL * max(1.0, np.abs(b).max()), (o, a, b)
            got = got.copy()
            got["glMatrix"][written] = want["glMatrix"][written]
        assert got.tobytes() == want.tobytes(), (o, np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))[:8].tolist())
        if not in_place:
            assert dm.cpu().numpy().tobytes() == recs.tobytes()


# ---- the chain on the device ------------------------------------------------------------------------------------------------------------

COLOUR = np.array([250, 10, 200, 255], np.uint8)   # R G B A


def test_the_chain_on_the_device(oa, L):
    """the feature end to end: the CPU chain's 1280 x 960 scenes delivered turned by ROT90_CW (960 x 1280), turned upright on the
    device (ROT270_CW), detected there with the upright camera, the records handed over on the device, carried back with ROT90_CW and
    drawn on the frames as they were delivered -- the oracle's markers on the upright frames, the upright frames themselves, the
    records mapped by numpy bit for bit, the host rendering under those records byte for byte.  Nothing crosses to the host between
    the upload and the downloads at the end"""
    import torch
    FW, FH = OR.CHAIN_FULL
    TW, TH = OR.oriented_size((FW, FH), "rot90")
    scenes = OR.chain_scenes()
    n = len(scenes)
    tpls = OR.chain_templates()
    cam = PS.camera(FW, FH)
    det = oa.Detector(FW, FH, max_batch=n)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    painter = oa.Detector(TW, TH, max_batch=1)     # render_records is bound by its context's size: a context for the turned frames
    overlay = np.broadcast_to(COLOUR, (4, 4, 4)).copy()
    painter.set_overlay(-1, overlay)
    upright = FK.pix_layout(n, FW, FH, "bgr", True)
    delivered = FK.pix_layout(n, TW, TH, "bgr", True)
    for f, sc in enumerate(scenes):
        upright.view(f)[...] = sc.frame
        delivered.view(f)[...] = OR.np_orient(sc.frame, "rot90")
    blank = FK.pix_layout(n, FW, FH, "bgr", True, fill=FK.GUARD)
    M = det.max_markers
    d_delivered, d_upright = to_device(delivered.buf), to_device(blank.buf)
    d_recs, d_counts = to_device(np.full(n * M * FK.MARKER_DTYPE.itemsize, FK.GUARD, np.uint8)), to_device(np.zeros(n, np.int32))
    d_back = to_device(np.full(n * M * FK.MARKER_DTYPE.itemsize, FK.GUARD, np.uint8))
    torch.cuda.synchronize()
    # one stream, nothing waited for in between
    s = det.stream_ptr()
    det.orient(d_delivered.data_ptr() + delivered.offset(0), TW, TH, d_upright.data_ptr() + blank.offset(0), n, "rot270", fmt="bgr",
               src_row_stride=delivered.row_stride, src_frame_stride=delivered.frame_stride, dst_row_stride=blank.row_stride,
               dst_frame_stride=blank.frame_stride)
    det.enqueue_device(d_upright.data_ptr() + blank.offset(0), FW, FH, n, row_stride=blank.row_stride, frame_stride=blank.frame_stride)
    det.results_to_device(d_recs.data_ptr(), d_counts.data_ptr())
    painter.orient_records(d_recs.data_ptr(), d_counts.data_ptr(), n, d_back.data_ptr(), (FW, FH), "rot90", per_frame=M, stream=s)
    painter.render_records(d_delivered.data_ptr() + delivered.offset(0), TW, TH, n, d_back.data_ptr(), d_counts.data_ptr(), per_frame=M, fmt="bgr",
                           row_stride=delivered.row_stride, frame_stride=delivered.frame_stride, stream=s)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    same(d_upright.cpu().numpy(), upright.buf, upright.pixel_mask(), "the upright frames")
    for f in range(n):
        ref = OracleFrame(np.ascontiguousarray(scenes[f].frame), tpls, cam, planes=False)
        assert len(ref.markers) == 1
        check_markers(f, ref, markers, counts, where="chain")
    recs = d_recs.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, M)
    assert all(recs[f, :counts[f]].tobytes() == markers[f, :counts[f]].tobytes() for f in range(n))
    want_back = np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, M).copy()
    for f in range(n):
        want_back[f, :counts[f]] = recs[f, :counts[f]]
        want_back["square"][f, :counts[f]] = OR.np_orient_squares(recs["square"][f, :counts[f]], (FW, FH), "rot90")
    rc, host_back = OR.host_orient_records(L, recs, counts, (FW, FH), "rot90", out=want_back)
    assert rc == 0 and host_back.tobytes() == want_back.tobytes()
    got_back = d_back.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, M)
    assert got_back.tobytes() == want_back.tobytes()
    for f in range(n):
        p = scenes[f].markers[0]
        truth = PS.PlantedMarker(OR.np_orient_points(p.quad, (FW, FH), "rot90"), p.R, p.t, p.template, p.tilt, p.size)
        m, kk, d = PS.match(got_back[f, 0]["square"], [truth])
        assert m is truth and kk is not None, (f, d)
    LO = OC.build_emul()
    rendered, drawn = OC.host_render(LO, delivered, want_back, counts, {-1: overlay})
    assert min(drawn) >= 1 and (rendered != delivered.buf).any()
    same(d_delivered.cpu().numpy(), rendered, delivered.pixel_mask(), "rendered")

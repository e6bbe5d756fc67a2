"""The projective warp on the device (ocvar_hip_warp / ocvar_hip_warp_records / ocvar_hip_board_plane_maps) byte for byte against the
host build of warp_core.h (tests/warp_chain.py): whole destination buffers are compared, the guard bytes in the row padding, between
the frames and around the block included, whole status and record blocks, the slots that are not written included, and the plane maps
to the last bit."""
import itertools

import numpy as np
import pytest

import board_chain as BC
import frame_kit as FK
import helpers as H
import persp_synth as PS
import undistort_chain as UC
import warp_chain as WC
from frame_kit import E_ARG, hand_made_records, oa, same, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4   # tests/test_gpu_parity.py: check_markers
# destination widths and heights on both sides of the kernel's tile, and two tiles and a pixel
WIDTHS = [WC.TILE_W - 1, WC.TILE_W, WC.TILE_W + 1, 2 * WC.TILE_W + 1]
HEIGHTS = sorted({h + d for h in WC.TILE_HS.values() for d in (-1, 0, 1)} | {2 * WC.TILE_H + 1})     # (both tile heights)
COMBOS = [(i, b) for i in (WC.LINEAR, WC.NEAREST) for b in (WC.CONSTANT, WC.REPLICATE)]
FILL = [7, 130, 255, 66]


@pytest.fixture(scope="module")
def L():
    return WC.build_emul()


@pytest.fixture(scope="module")
def det(oa):
    return oa.Detector(64, 32, max_batch=1)   # (neither the sizes nor n_frames are bound by the context's)


def device_warp(det, src, dst, maps, interp=WC.LINEAR, border=WC.CONSTANT, fill=None, flags=0, with_status=True):
    """det.warp on device copies of src.buf, dst.buf and the maps -> (destination buffer, status [n], source buffer afterwards)"""
    import torch
    d, dd, dm = to_device(src.buf), to_device(dst.buf), to_device(WC.maps_array(maps))
    ds = to_device(np.full(dst.n, -7, np.int32))
    assert d.data_ptr() % 4 == 0 and dd.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    det.warp(d.data_ptr() + src.offset(0), src.width, src.height, dd.data_ptr() + dst.offset(0), dst.width, dst.height, dst.n, dm.data_ptr(),
             interp={v: k for k, v in WC.INTERPS.items()}[interp], border={v: k for k, v in WC.BORDERS.items()}[border], fill=fill,
             inverse_map=bool(flags & WC.INVERSE_MAP), one_map=bool(flags & WC.ONE_MAP), fmt=dst.fmt, src_row_stride=src.row_stride,
             src_frame_stride=src.frame_stride, dst_row_stride=dst.row_stride, dst_frame_stride=dst.frame_stride,
             d_status_ptr=ds.data_ptr() if with_status else None)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), ds.cpu().numpy().view(np.int32), d.cpu().numpy()


def check(L, det, src, dst, maps, interp, border, fill, flags, where, want_status=None):
    rc, want, status = WC.host_warp(L, src, dst, maps, interp, border, fill, flags)
    assert rc >= 0 and (want[~dst.pixel_mask()] == FK.GUARD).all()
    if want_status is not None:
        assert status.tolist() == want_status, where
    got, got_status, src_after = device_warp(det, src, dst, maps, interp, border, fill, flags)
    assert (src_after == src.buf).all(), where
    assert got_status.tolist() == status.tolist(), where
    same(got, want, dst.pixel_mask(), where)
    return got


def inverse_maps(src_size, dst_size):
    """destination -> source maps, one per frame of a call: the shared maps (forward ones inverted here, in numpy), and in the third
    place one that is not finite, whose frame is skipped"""
    shared = WC.shared_maps(src_size, dst_size)
    out = []
    for name in ("mild", "magnify", "tilted", "horizon", "outside", "fit"):
        m, flags = shared[name]
        out.append(m if flags & WC.INVERSE_MAP else WC.np_invert(m))
    out.insert(2, WC.SKIPPED_MAPS["nan"])
    return out, [1, 1, 0, 1, 1, 1, 1]


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FK.FMTS)
def test_warp_sweep(oa, L, det, fmt):
    """destination widths x heights around the tile, seven frames with a map each (one of them skipped), both interpolations and both
    borders in turn, on the dword path (everything a multiple of 4) and on the byte path (an odd lead, odd paddings, a frame gap of 5):
    the host core's buffer and status each time, the same pixels on both paths, the source untouched"""
    src_size = (90, 60)
    for k, ((iw, dw), (ih, dh)) in enumerate(itertools.product(enumerate(WIDTHS), enumerate(HEIGHTS))):
        interp, border = COMBOS[(iw + ih) % 4]     # (every pair meets every width and, the heights being more than four, every height)
        maps, status = inverse_maps(src_size, (dw, dh))
        where = "%s %dx%d interp %d border %d" % (fmt, dw, dh, interp, border)
        pixels = []
        for aligned in (True, False):
            src = FK.pix_layout(len(maps), *src_size, fmt, aligned, seed=dw + k)
            dst = WC.dst_layout(src, (dw, dh), aligned)
            got = check(L, det, src, dst, maps, interp, border, FILL, WC.INVERSE_MAP, where + " aligned=%s" % aligned, status)
            pixels.append(np.stack([dst.view(f, got) for f in range(dst.n)]))
        assert (pixels[0] == pixels[1]).all(), where


@pytest.mark.parametrize("interp,border", COMBOS)
def test_forward_maps_and_one_map(oa, L, det, interp, border):
    """forward maps, inverted on the device: per frame, a singular one among them, and one map for every frame; with and without a
    status block; a NULL fill is zeros"""
    src_size, dst_size = (90, 60), (WC.TILE_W + 9, 2 * WC.TILE_H + 3)
    shared = WC.shared_maps(src_size, dst_size)
    maps = [shared["mild"][0], WC.SKIPPED_MAPS["singular"], shared["magnify"][0], shared["shift"][0], shared["identity"][0]]
    for fmt, aligned in (("bgr", True), ("gray", False), ("rgba", False)):
        src = FK.pix_layout(len(maps), *src_size, fmt, aligned, seed=3)
        dst = WC.dst_layout(src, dst_size, aligned)
        check(L, det, src, dst, maps, interp, border, FILL, 0, "forward %s" % fmt, [1, 0, 1, 1, 1])
        got = check(L, det, src, dst, maps[0], interp, border, None, WC.ONE_MAP, "one map %s" % fmt, [1] * 5)
        rc, want, _ = WC.host_warp(L, src, dst, maps[0], interp, border, [0, 0, 0, 0], WC.ONE_MAP)
        assert (got == want).all()
        got2, status, _ = device_warp(det, src, dst, maps, interp, border, FILL, 0, with_status=False)
        rc, want2, _ = WC.host_warp(L, src, dst, maps, interp, border, FILL, 0)
        same(got2, want2, dst.pixel_mask(), "no status block")
        assert (status == -7).all()


def test_smallest_frames_and_a_source_narrower_than_a_dword(oa, L, det):
    for (sw, sh), (dw, dh) in [((1, 1), (1, 1)), ((2, 1), (1, 1)), ((1, 1), (2, 1)), ((2, 1), (2, 1)), ((3, 1), (5, 2)), ((1, 3), (2, 5)), ((3, 2), (WC.TILE_W + 1, 3))]:
        maps = [np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), np.array([0.5, 0, 0.25, 0, 0.5, 0.125, 0, 0, 1.0]), np.array([1, 0, -0.5, 0, 1, 0, 0.25, 0, 1.0])]
        for fmt, aligned in itertools.product(("gray", "bgr", "bgra"), (True, False)):
            for interp, border in COMBOS:
                src = FK.pix_layout(len(maps), sw, sh, fmt, aligned, seed=sw + dw)
                dst = WC.dst_layout(src, (dw, dh), aligned)
                check(L, det, src, dst, maps, interp, border, [1, 2, 3, 4], WC.INVERSE_MAP, "%dx%d -> %dx%d %s %s" % (sw, sh, dw, dh, fmt, aligned), [1, 1, 1])


# ---- the two classes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(WC.PLAN_CASES))
def test_both_classes_give_the_core_bytes(oa, L, case):
    """the cases whose classes tests/test_warp_cpu.py counts -- a magnifying map (staged), 300 x 200 shrunk into 8 x 8 (direct), a
    horizon across the destination (both), the whole destination outside the source -- and the same calls with every tile made direct
    by the tuning switch: the host core's bytes either way"""
    src_size, dst_size, name, classes = WC.PLAN_CASES[case]
    m, flags = WC.shared_maps(src_size, dst_size)[name]
    det = oa.Detector(64, 32, max_batch=1)
    for fmt in ("bgr", "rgba", "gray"):
        c = WC.plan_counts(L, m, src_size, dst_size, FK.BPP[FK.FORMATS[fmt]], WC.LINEAR, WC.CONSTANT, flags)
        assert (c["staged"] >= 1) == (classes in ("staged", "both")) and (c["direct"] >= 1) == (classes in ("direct", "both")), (case, fmt, c)
        for (interp, border), aligned in zip(COMBOS, (True, False, True, False)):
            src = FK.pix_layout(2, *src_size, fmt, aligned, seed=5)
            dst = WC.dst_layout(src, dst_size, aligned)
            for direct in (0, 1):
                det.set_tuning(warp_direct=direct)
                check(L, det, src, dst, m, interp, border, FILL, flags | WC.ONE_MAP, "%s %s direct=%d" % (case, fmt, direct), [1, 1])
    det.set_tuning(warp_direct=0)


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------

def test_more_frames_than_one_launch_takes(oa, L, det):
    """65537 frames of 2 x 1 GRAY pixels swapped by their own maps, every 1000th map not finite, stored without a gap: two launches
    (the grid's z ends at 65535), every frame once, maps and status of the second launch from the right place"""
    import torch
    n, lead = 65537, 64
    rng = np.random.default_rng(2)
    src = np.full(lead + 2 * n + lead, FK.GUARD, np.uint8)
    src[lead:lead + 2 * n] = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    dst = np.full(lead + 2 * n + lead, FK.GUARD, np.uint8)
    maps = np.tile(np.array([-1, 0, 1, 0, 1, 0, 0, 0, 1.0]), (n, 1))
    maps[1::2] = [1, 0, 0, 0, 1, 0, 0, 0, 1.0]
    maps[::1000, 4] = np.nan
    want, want_status = dst.copy(), np.full(n, -7, np.int32)
    assert L.warp_emul(src.ctypes.data + lead, 2, 1, 2, 2, want.ctypes.data + lead, 2, 1, 2, 2, n, FK.FORMATS["gray"], maps.ctypes.data, WC.LINEAR,
                       WC.CONSTANT, None, WC.INVERSE_MAP, want_status.ctypes.data) == n - len(range(0, n, 1000))
    d, dd, dm, ds = to_device(src), to_device(dst), to_device(maps), to_device(np.full(n, -7, np.int32))
    torch.cuda.synchronize()
    det.warp(d.data_ptr() + lead, 2, 1, dd.data_ptr() + lead, 2, 1, n, dm.data_ptr(), inverse_map=True, fmt="gray", d_status_ptr=ds.data_ptr())
    torch.cuda.synchronize()
    got = dd.cpu().numpy()
    assert (got == want).all(), np.flatnonzero(got != want)[:4].tolist()
    assert (ds.cpu().numpy().view(np.int32) == want_status).all()
    pairs, spairs = got[lead:lead + 2 * n].reshape(n, 2), src[lead:lead + 2 * n].reshape(n, 2)
    assert (pairs[65536] == spairs[65536][::-1]).all() and (pairs[65535] == spairs[65535]).all() and (pairs[65000] == FK.GUARD).all()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import ctypes as C
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(32, 16, max_batch=1)
    ctx = det._ctx
    SW, SH, DW, DH, n = 64, 32, 48, 40, 2
    src_h = np.full(n * 4 * SW * SH + 64, 77, np.uint8)
    dst_h = np.full(n * 4 * DW * DH + 64, FK.GUARD, np.uint8)
    maps_h = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1))
    ds, dd, dm, dst_ = to_device(src_h), to_device(dst_h), to_device(maps_h), to_device(np.full(n, -7, np.int32))
    torch.cuda.synchronize()
    sp, dp, mp, stp = ds.data_ptr(), dd.data_ptr(), dm.data_ptr(), dst_.data_ptr()
    span_s = (2 ** 31) // (SH - 1) + 1      # a row stride with which the rows of the source span more than 2^31 - 1 bytes
    span_d = (2 ** 31) // (DH - 1) + 1
    fill = (C.c_uint8 * 4)(1, 2, 3, 4)

    def call(**kw):
        a = dict(src=sp, sw=SW, sh=SH, srs=3 * SW, dst=dp, dw=DW, dh=DH, drs=3 * DW, n=n, fmt=0, maps=mp, interp=1, border=0, fill=fill, flags=0, status=stp)
        a.update(kw)
        return lib.ocvar_hip_warp(ctx, a["src"], a["sw"], a["sh"], a["srs"], a.get("sfs", a["srs"] * max(a["sh"], 1)), a["dst"], a["dw"], a["dh"], a["drs"],
                                  a.get("dfs", a["drs"] * max(a["dh"], 1)), a["n"], a["fmt"], a["maps"], a["interp"], a["border"], a["fill"], a["flags"],
                                  a["status"], None)

    cases = [dict(src=None), dict(dst=None), dict(maps=None), dict(fmt=5), dict(fmt=-1), dict(interp=2), dict(interp=-1), dict(border=2), dict(border=-1),
             dict(flags=4), dict(flags=8), dict(flags=-1),
             dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=-1), dict(sw=32768, srs=3 * 32768), dict(sh=32768), dict(dw=32768, drs=3 * 32768), dict(dh=32768),
             dict(srs=3 * SW - 1), dict(drs=3 * DW - 1), dict(fmt=2, srs=4 * SW - 1, drs=4 * DW), dict(fmt=2, srs=4 * SW, drs=4 * DW - 1), dict(fmt=4, srs=SW, drs=DW - 1),
             dict(srs=span_s, sfs=3 * SW * SH, n=1), dict(drs=span_d, dfs=3 * DW * DH, n=1),
             dict(n=0), dict(n=-1),
             dict(dst=sp), dict(dst=sp + 3 * SW * SH * n - 1), dict(src=dp + 3 * DW * DH * n - 1), dict(src=dp + 1)]
    for rounds in range(2):
        for kw in cases:
            assert call(**kw) == E_ARG, kw
            assert lib.ocvar_hip_last_error(ctx), kw
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == dst_h).all() and (ds.cpu().numpy() == src_h).all() and (dst_.cpu().numpy().view(np.int32) == -7).all()
    for bad in (dict(interp="cubic"), dict(border="reflect"), dict(interp=1), dict(fill=[1, 2, 3, 4, 5]), dict(fill=[256])):
        with pytest.raises(ValueError):
            det.warp(sp, SW, SH, dp, DW, DH, n, mp, **bad)
    # after all that the context still warps; a source larger than the context's maximum all along; fill and status may be NULL
    assert call(fill=None, status=None) == 0 and call() == 0
    torch.cuda.synchronize()
    want = dst_h.copy()
    assert L.warp_emul(src_h.ctypes.data, SW, SH, 3 * SW, 3 * SW * SH, want.ctypes.data, DW, DH, 3 * DW, 3 * DW * DH, n, 0, maps_h.ctypes.data, 1, 0, fill, 0, None) == n
    assert (dd.cpu().numpy() == want).all() and dst_.cpu().numpy().view(np.int32).tolist() == [1, 1]

    # warp_records
    recs = to_device(np.zeros(2 * 4, FK.MARKER_DTYPE))
    counts = to_device(np.array([4, 4], np.int32))
    before = recs.cpu().numpy().copy()

    def rcall(**kw):
        a = dict(m=recs.data_ptr(), c=counts.data_ptr(), n=2, per=4, maps=mp, flags=0, out=recs.data_ptr())
        a.update(kw)
        return lib.ocvar_hip_warp_records(ctx, a["m"], a["c"], a["n"], a["per"], a["maps"], a["flags"], a["out"], None)

    rcases = [dict(m=None), dict(c=None), dict(maps=None), dict(out=None), dict(n=0), dict(n=-1), dict(per=0), dict(per=det.max_markers + 1),
              dict(flags=8), dict(flags=-1), dict(flags=1), dict(flags=3), dict(flags=4), dict(flags=6)]   # (1: the inverse map; 4: no camera is set)
    for kw in rcases:
        assert rcall(**kw) == E_ARG, kw
        assert lib.ocvar_hip_last_error(ctx), kw
    # board_plane_maps
    poses = to_device(np.zeros(2, oa.BOARD_DTYPE))
    out = to_device(np.full(18, 5.0))
    rect = (C.c_double * 4)(0, 0, 4, 3)

    def bcall(**kw):
        a = dict(p=poses.data_ptr(), n=2, rect=rect, dw=64, dh=48, maps=out.data_ptr())
        a.update(kw)
        return lib.ocvar_hip_board_plane_maps(ctx, a["p"], a["n"], a["rect"], a["dw"], a["dh"], a["maps"], None)

    bcases = [dict(), dict(p=None), dict(rect=None), dict(maps=None), dict(n=0), dict(dw=0), dict(dh=32768)]     # (the first: no camera is set)
    for kw in bcases:
        assert bcall(**kw) == E_ARG, kw
        assert lib.ocvar_hip_last_error(ctx), kw
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(DW, DH))))
    for kw in bcases[1:]:
        assert bcall(**kw) == E_ARG, kw
    for kw in (dict(flags=1), dict(flags=5), dict(flags=8)):
        assert rcall(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert (recs.cpu().numpy() == before).all() and (out.cpu().numpy().view(np.float64) == 5.0).all()
    assert rcall() == 0 and rcall(flags=4) == 0 and rcall(flags=2) == 0 and bcall() == 0
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy().view(np.float64)).all()      # (poses of status 0)


def test_a_context_that_never_warps_allocates_nothing(oa):
    """device memory in use does not change over a context's first warps, record maps and plane maps (as tests/test_gpu_yuv.py shows
    it for the conversions): there is no workspace, and a context that never calls them has nothing of theirs"""
    import torch
    n, W, Hh = 2, 64, 48
    src, dst = to_device(np.zeros(n * W * Hh * 3, np.uint8)), to_device(np.zeros(n * W * Hh * 3, np.uint8))
    maps = to_device(np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1)))
    recs, counts = to_device(np.zeros(n * 4, FK.MARKER_DTYPE)), to_device(np.array([4, 4], np.int32))
    poses = to_device(np.zeros(n, oa.BOARD_DTYPE))

    def run(det):
        det.warp(src.data_ptr(), W, Hh, dst.data_ptr(), W, Hh, n, maps.data_ptr(), fmt="bgr")
        det.warp_records(recs.data_ptr(), counts.data_ptr(), n, recs.data_ptr(), maps.data_ptr(), per_frame=4)
        det.board_plane_maps(poses.data_ptr(), n, (0, 0, 4, 3), W, Hh, maps.data_ptr())
        torch.cuda.synchronize()

    warm = oa.Detector(W, Hh, max_batch=n)
    warm.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
    run(warm)      # (the kernels' code is loaded now)
    for attempt in range(3):
        det = oa.Detector(W, Hh, max_batch=n)
        det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        run(det)
        after = torch.cuda.mem_get_info()[0]
        if after == before:
            break
    assert after == before, (before, after)


# ---- warp_records -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("slots,in_place,one_map", [(1, True, False), (5, False, True), ("all", True, True), ("all", False, False)])
def test_warp_records(oa, L, pose, slots, in_place, one_map):
    """counts of 0, 1, per_frame and more; a map per frame and one for all; into the block itself and into another one, whose other
    slots keep their guard bytes; every field but the square (and glMatrix with the pose flag) bit for bit as it was, the square the
    host core's bits (and numpy's), glMatrix the host pose core's on the new square within check_markers' tolerance"""
    import torch
    size = (640, 480)
    det = oa.Detector(64, 32, max_batch=1)
    slots = det.max_markers if slots == "all" else slots
    n = 4
    cam = PS.camera(*size, lens=True)
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    K = np.array(list(cam.cameraMatrix)).reshape(3, 3)
    # the homographies small turns of the camera induce: the hand-made squares stay the well-conditioned views of a square they are
    maps = np.stack([(K @ BC.rodrigues(np.array([0.05, -0.08, 0.2]) * (f + 1) / n) @ np.linalg.inv(K)).reshape(9) for f in range(n)])
    if not pose:
        maps[1] = [2, 0, 1, 0, 2, 3, 1, 0, -0.25]
    if one_map:
        maps = maps[:1]
    recs = hand_made_records(np.random.default_rng(slots), n, slots, *size, frame_corners=False)
    if not pose:
        recs["square"][1, 0, :2] = [0.25, 9]        # on the horizon of maps[1]
        if slots >= 4:
            recs["square"][2, 1, 3] = np.nan
            recs["square"][2, 2, 0] = 1e30
    given = [0, 1, slots, slots + 3]
    live = np.minimum(given, slots)
    flags = (WC.ONE_MAP if one_map else 0) | (WC.POSE if pose else 0)
    rc, want_new = WC.host_warp_records(L, recs, live, maps, flags, cam=cam)
    assert rc == 0
    written = np.arange(slots)[None, :] < live[:, None]
    guard = np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(n, slots)
    before = recs.copy() if in_place else guard.copy()
    want = before.copy()
    want[written] = want_new[written]
    np_sq = np.stack([WC.np_warp_squares(recs["square"][f], maps[0 if one_map else f]) for f in range(n)])
    assert want_new["square"][written].view(np.uint32).tolist() == np_sq[written].view(np.uint32).tolist()
    dm, dc, dmaps = to_device(recs), to_device(np.asarray(given, np.int32)), to_device(maps)
    do = dm if in_place else to_device(before)
    torch.cuda.synchronize()
    det.warp_records(dm.data_ptr(), dc.data_ptr(), n, do.data_ptr(), dmaps.data_ptr(), per_frame=slots, one_map=one_map, pose=pose)
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


# ---- the board's plane --------------------------------------------------------------------------------------------------------------------

def test_board_plane_maps_to_the_last_bit(oa, L):
    """poses of every kind -- solved ones at tilts up to 60 degrees, no rotation at all, status 0 and -1, numbers that are not finite --
    and rectangles that flip, collapse to a pixel and have no extent: the host core's doubles, bit for bit"""
    import torch
    rng = np.random.default_rng(8)
    cam = PS.camera(1920, 1080)
    K = np.array(list(cam.cameraMatrix)).reshape(3, 3)
    det = oa.Detector(64, 32, max_batch=1)
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    poses = []
    for k in range(70):
        r = rng.normal(size=3)
        r *= np.radians(rng.uniform(0, 60)) / np.linalg.norm(r)
        poses.append(WC.board_pose(BC.rodrigues(r), [rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(5, 30)]))
    poses.append(WC.board_pose(np.eye(3), [0, 0, 10]))
    poses += [WC.board_pose(np.eye(3), [0, 0, 10], status=0), WC.board_pose(np.eye(3), [0, 0, 10], status=-1), WC.board_pose(np.eye(3), [np.nan, 0, 10]),
              WC.board_pose(np.eye(3), [0, np.inf, 10])]
    raw = np.frombuffer(b"".join(bytes(p) for p in poses), np.uint8).copy()
    n = len(poses)
    dp = to_device(raw)
    for rect, size in [((-0.5, -0.5, 6.0, 4.5), (521, 401)), ((0, 4, 5.5, 0), (300, 200)), ((1, 1, 2, 2), (1, 1)), ((1, 1, 1, 3), (1, 7)), ((1, 0, 1, 4), (64, 48)),
                       ((0, 0, np.nan, 4), (64, 48))]:
        want = WC.host_plane_maps(L, raw, K, rect, size)
        out = to_device(np.full(9 * n + 2, 5.0))
        torch.cuda.synchronize()
        det.board_plane_maps(dp.data_ptr(), n, rect, size[0], size[1], out.data_ptr() + 8)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.float64)
        assert got[0] == 5.0 and got[-1] == 5.0
        got = got[1:-1].reshape(n, 9)
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (rect, size, len(bad), bad[:4].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
        assert np.isnan(want[-4:]).all() and (np.isfinite(want[:71]).all() or rect[0] == rect[2] or not np.isfinite(rect).all())


# ---- the chain on the device ------------------------------------------------------------------------------------------------------------

def test_the_chain_on_the_device(oa, L):
    """the feature end to end on one stream, nothing waited for in between: frames of a camera with a lens undistorted, detected with
    the board by a context with the pinhole camera of the same matrix, the board poses handed over on the device, the plane maps, the
    warp to bird's-eye frames.  Against the CPU chain: the undistorted frames byte for byte, the device's poses within the board
    tests' tolerance of the host board core's, the plane maps bit for bit and the bird's-eye frames byte for byte from the device's
    own poses, and on those frames the oracle finds every marker of the board where the layout puts it"""
    import torch
    from test_gpu_board import check_against_host
    W, Hh = 1920, 1080
    lens_cam, cam = PS.camera(W, Hh, lens=True), PS.camera(W, Hh)
    names, board, sc = WC.chain_scenes(2, lens_cam)
    n = len(sc)
    tpls = H.oracle_templates(names)
    rect, size = WC.chain_rect(board)
    Lu, Lb = UC.build_emul(), BC.build_emul()
    lens = oa.Detector(W, Hh, max_batch=1)      # (the context with the lens: undistort is bound by its context's size)
    lens.set_camera(oa.Camera.from_buffer_copy(bytes(lens_cam)))
    det = oa.Detector(W, Hh, max_batch=n)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    det.set_board(board)
    taken = FK.pix_layout(n, W, Hh, "bgr", True)
    for f in range(n):
        taken.view(f)[...] = sc[f][0]
    flat = FK.pix_layout(n, W, Hh, "bgr", True, fill=FK.GUARD)
    top = FK.pix_layout(n, size[0], size[1], "bgr", True, fill=FK.GUARD)
    d_taken, d_flat, d_top = to_device(taken.buf), to_device(flat.buf), to_device(top.buf)
    d_poses, d_maps, d_status = to_device(np.zeros(n, oa.BOARD_DTYPE)), to_device(np.zeros(9 * n)), to_device(np.full(n, -7, np.int32))
    torch.cuda.synchronize()
    s = det.stream_ptr()
    lens.undistort(d_taken.data_ptr() + taken.offset(0), d_flat.data_ptr() + flat.offset(0), W, Hh, n, fmt="bgr", src_row_stride=taken.row_stride,
                   src_frame_stride=taken.frame_stride, dst_row_stride=flat.row_stride, dst_frame_stride=flat.frame_stride, stream=s)
    det.enqueue_device(d_flat.data_ptr() + flat.offset(0), W, Hh, n, row_stride=flat.row_stride, frame_stride=flat.frame_stride)
    det.board_poses_to_device(d_poses.data_ptr())
    det.board_plane_maps(d_poses.data_ptr(), n, rect, size[0], size[1], d_maps.data_ptr())
    det.warp(d_flat.data_ptr() + flat.offset(0), W, Hh, d_top.data_ptr() + top.offset(0), size[0], size[1], n, d_maps.data_ptr(), fill=[220, 220, 220],
             inverse_map=True, fmt="bgr", src_row_stride=flat.row_stride, src_frame_stride=flat.frame_stride, dst_row_stride=top.row_stride,
             dst_frame_stride=top.frame_stride, d_status_ptr=d_status.data_ptr())
    markers, counts = det.collect()
    torch.cuda.synchronize()
    want_flat = UC.host_undistort(Lu, taken, lens_cam, flat)
    got_flat = d_flat.cpu().numpy()
    same(got_flat, want_flat, flat.pixel_mask(), "the undistorted frames")
    poses = d_poses.cpu().numpy().view(oa.BOARD_DTYPE)
    assert poses.tobytes() == det.board_poses().tobytes() and (poses["status"] == 1).all() and (poses["n_markers"] == len(board)).all()
    check_against_host(Lb, det, markers, counts, poses, board, tpls, cam, where="chain")
    K = np.array(list(cam.cameraMatrix)).reshape(3, 3)
    want_maps = WC.host_plane_maps(L, poses, K, rect, size)
    got_maps = d_maps.cpu().numpy().view(np.float64).reshape(n, 9)
    assert (got_maps.view(np.uint64) == want_maps.view(np.uint64)).all()
    flat_frames = FK.pix_layout(n, W, Hh, "bgr", True)
    flat_frames.buf[...] = want_flat
    rc, want_top, status = WC.host_warp(L, flat_frames, top, want_maps, WC.LINEAR, WC.CONSTANT, [220, 220, 220], WC.INVERSE_MAP)
    assert rc == n and d_status.cpu().numpy().view(np.int32).tolist() == [1] * n
    got_top = d_top.cpu().numpy()
    same(got_top, want_top, top.pixel_mask(), "the bird's-eye frames")
    for f in range(n):
        found, _, _ = H.oracle_registration(np.ascontiguousarray(top.view(f, got_top)), tpls, PS.camera(*size))
        errs = WC.corner_errors(found, board, rect, size)
        assert sorted(errs) == [tid for tid, _ in board] and max(errs.values()) <= WC.CHAIN_BAR_PX, (f, errs)

"""Flow tracking on the device (ocvar_hip_flow_records) byte for byte against the host build of flow_core.h (tests/flow_chain.py):
whole record blocks, the slots that are not written included, every status and the bits of every error; glMatrix under
OCVAR_FLOW_POSE within the tolerance tests/test_gpu_parity.py uses for poses (device libm).  The frames are compared too: flow only
reads them."""
import ctypes as C

import numpy as np
import pytest

import flow_chain as FC
import frame_kit as FK
import helpers as H
from frame_kit import E_ARG, oa, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4   # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def L():
    return FC.build_emul()


@pytest.fixture(scope="module")
def det128(oa):
    """a context of max_batch 2: three frames go through the workspace in two chunks"""
    return oa.Detector(128, 96, max_batch=2)


def guard_like(recs):
    return np.frombuffer(np.full(recs.nbytes, FK.GUARD, np.uint8).tobytes(), FK.MARKER_DTYPE).reshape(recs.shape).copy()


def device_flow(det, prev, nxt, recs, counts, p, in_place=False, with_status=True, with_err=True, odd=False, stream=None, out=None):
    """det.flow_records on device copies -> (records, status or None, err or None); the frames must come back unchanged"""
    import torch
    n, slots = recs.shape
    dp, dn = to_device(prev.buf, odd), to_device(nxt.buf, odd)
    dm, dc = to_device(recs), to_device(np.asarray(counts, np.int32))
    do = dm if in_place else to_device(guard_like(recs) if out is None else out)
    ds = to_device(np.full(n * slots * 4, FK.GUARD, np.uint8)) if with_status else None
    de = to_device(np.full(n * slots * 16, FK.GUARD, np.uint8)) if with_err else None
    assert (dp.data_ptr() % 4 == 1) == odd
    torch.cuda.synchronize()
    det.flow_records(dp.data_ptr() + prev.offset(0), dn.data_ptr() + nxt.offset(0), prev.width, prev.height, n, dm.data_ptr(), dc.data_ptr(),
                     do.data_ptr(), per_frame=slots, fmt=prev.fmt, prev_row_stride=prev.row_stride, prev_frame_stride=prev.frame_stride,
                     next_row_stride=nxt.row_stride, next_frame_stride=nxt.frame_stride, params=p,
                     d_status_ptr=ds.data_ptr() if with_status else None, d_err_ptr=de.data_ptr() if with_err else None, stream=stream)
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == prev.buf).all() and (dn.cpu().numpy() == nxt.buf).all()
    if not in_place:
        assert dm.cpu().numpy().tobytes() == recs.tobytes()
    return (do.cpu().numpy().view(FK.MARKER_DTYPE).reshape(n, slots),
            ds.cpu().numpy().view(np.int32).reshape(n, slots) if with_status else None,
            de.cpu().numpy().view(np.float32).reshape(n, slots, 4) if with_err else None)


def same(got, want, where, pose=False):
    gr, gs, ge = got
    wr, ws, we = want
    if gs is not None:
        assert (gs == ws).all(), (where, gs.tolist(), ws.tolist())
    if ge is not None:
        assert ge.tobytes() == we.tobytes(), (where, ge[ge.view(np.uint32) != we.view(np.uint32)][:4], we[ge.view(np.uint32) != we.view(np.uint32)][:4])
    if pose:
        for name in ("templateId", "markerId", "score", "square", "aspectRatio"):
            assert gr[name].tobytes() == wr[name].tobytes(), (where, name)
        g, w = gr["glMatrix"], wr["glMatrix"]
        tracked = ws == 1
        assert g[~tracked].tobytes() == w[~tracked].tobytes(), where
        for a, b in zip(g[tracked], w[tracked]):
            assert np.abs(a - b).max() <= POSE_RTOL * max(1.0, np.abs(b).max()), (where, a, b)
    else:
        assert gr.tobytes() == wr.tobytes(), (where, gr["square"][(gr["square"] != wr["square"]).any(-1)][:2], wr["square"][(gr["square"] != wr["square"]).any(-1)][:2])


def quads(rng, n, slots, W, Hh, margin):
    """[n, slots] records with every field filled: convex quads well inside the frame, one corner of the last slot outside it"""
    cx, cy = rng.uniform(margin, W - margin, (n, slots, 1)), rng.uniform(margin, Hh - margin, (n, slots, 1))
    r = min(W, Hh) / 5.0
    ang = np.deg2rad([225, 315, 45, 135]) + rng.uniform(-0.3, 0.3, (n, slots, 4))
    rad = rng.uniform(0.6 * r, r, (n, slots, 4))
    sq = np.stack([np.clip(cx + rad * np.cos(ang), 0, W - 1), np.clip(cy + rad * np.sin(ang), 0, Hh - 1)], -1).reshape(n * slots, 8)
    recs = FK.records(sq, template_ids=rng.integers(0, 9, n * slots), scores=rng.integers(0, 2, n * slots)).reshape(n, slots)
    recs["glMatrix"] = rng.normal(size=(n, slots, 16))
    recs["aspectRatio"] = rng.uniform(0.5, 2, (n, slots))
    recs["square"][-1, -1, 2] = W + 3.5
    return recs


def textured(rng, n, W, Hh, fmt, shift, row_pad=0, frame_gap=0, cell=6):
    """(prev, next): Frames blocks whose grey is a texture and its shift; in a colour format the channels differ"""
    prev = FK.Frames(n, W, Hh, fmt, row_pad=row_pad, frame_gap=frame_gap, seed=1)
    nxt = FK.Frames(n, W, Hh, fmt, row_pad=row_pad + 1, frame_gap=frame_gap + 3, seed=2)
    for f in range(n):
        A, B = FC.shifted_pair(rng, W, Hh, shift[0] + f, shift[1], cell=cell)
        for fr, g in ((prev, A), (nxt, B)):
            v = fr.view(f)
            for c in range(min(fr.bpp, 3)):
                v[..., c] = np.clip(g.astype(np.int64) + 9 * c - 9, 0, 255)   # (byte 3 of a four-channel pixel stays random)
    return prev, nxt


def test_levels_clipped_by_the_window_rule(L, det128):
    """37 x 29 grey, one frame, levels 5, w = 1: L = 2 (level 3 is 5 x 4); rows that end inside a lane's dword on every level"""
    assert FC.host_geom(L, 37, 29, 1, 5)[0] == 2
    rng = np.random.default_rng(21)
    prev, nxt = textured(rng, 1, 37, 29, "gray", (1, -1), cell=2)
    recs = quads(rng, 1, 4, 37, 29, 9)
    p = FC.params(half_win=1, levels=5)
    want = FC.host_flow(L, prev, nxt, recs, [4], p)
    assert (want[1][0, :3] == 1).any() and want[1][0, 3] == -1
    same(device_flow(det128, prev, nxt, recs, [4], p), (guard_merge(want, recs, [4]),) + want[1:], "37x29")


def guard_merge(want, recs, counts):
    """the records a guard-filled output block holds after the call: the host build's in the live slots"""
    out = guard_like(recs)
    live = np.arange(recs.shape[1])[None, :] < np.minimum(counts, recs.shape[1])[:, None]
    out[live] = want[0][live]
    return out


@pytest.mark.parametrize("fmt", FK.FMTS)
def test_formats_strides_counts_and_chunks(L, det128, fmt):
    """96 x 64, three frames on a context of two: padded rows, an odd base address, a gap between the frames; counts 0, 1 and one above
    records_per_frame"""
    rng = np.random.default_rng(22)
    n, slots, W, Hh = 3, 3, 96, 64
    prev, nxt = textured(rng, n, W, Hh, fmt, (2, 1), row_pad=5, frame_gap=11)
    recs = quads(rng, n, slots, W, Hh, 22)
    counts = [0, 1, slots + 2]
    p = FC.params(half_win=4, levels=2)
    want = FC.host_flow(L, prev, nxt, recs, counts, p)
    assert want[1].tolist()[0] == [0, 0, 0] and want[1][1, 0] == 1 and want[1][2, 2] == -1 and (want[1][2, :2] == 1).all()
    same(device_flow(det128, prev, nxt, recs, counts, p, odd=True), (guard_merge(want, recs, counts),) + want[1:], fmt + " odd address")
    if fmt in ("bgr", "gray"):   # (the dword loads of the grey kernel need an aligned block: strides that are multiples of 4)
        pa, na = textured(rng, n, W, Hh, fmt, (2, 1), row_pad=4 if fmt == "gray" else 12, frame_gap=8)
        na = FK.Frames(n, W, Hh, fmt, row_pad=pa.row_stride - W * pa.bpp, frame_gap=8, seed=5)
        for f in range(n):
            na.view(f)[...] = np.roll(pa.view(f), (1, 2), (0, 1))
        assert pa.row_stride % 4 == 0 and pa.frame_stride % 4 == 0 and na.row_stride % 4 == 0 and na.frame_stride % 4 == 0
        want = FC.host_flow(L, pa, na, recs, counts, p)
        same(device_flow(det128, pa, na, recs, counts, p), (guard_merge(want, recs, counts),) + want[1:], fmt + " aligned")


@pytest.mark.parametrize("max_iter", [1, 100])
def test_largest_window_and_all_levels(oa, L, max_iter):
    """641 x 479 BGR, levels 5, w = 15: 35 KB of LDS, odd sides on every level, one step and a hundred"""
    rng = np.random.default_rng(23)
    W, Hh = 641, 479
    det = oa.Detector(W, Hh, max_batch=1)
    prev, nxt = textured(rng, 1, W, Hh, "bgr", (5, -3), cell=8)
    recs = quads(rng, 1, 6, W, Hh, 120)
    p = FC.params(half_win=15, levels=5, max_iter=max_iter, eps=0.0)
    assert FC.host_geom(L, W, Hh, 15, 5)[0] == 3   # (level 4 is 41 x 30: below 33)
    want = FC.host_flow(L, prev, nxt, recs, [6], p)
    assert (want[1][0, :5] == 1).all()
    same(device_flow(det, prev, nxt, recs, [6], p), want, "641x479 max_iter %d" % max_iter)
    det.close()


def test_one_more_frame_than_a_chunk(oa, L):
    """64 x 48 grey, 33 frames on a context of max_batch 40: the workspace holds 32"""
    rng = np.random.default_rng(24)
    n, slots, W, Hh = 33, 2, 64, 48
    det = oa.Detector(W, Hh, max_batch=40)
    prev, nxt = textured(rng, n, W, Hh, "gray", (-14, 1), cell=4)   # (the shift grows by one per frame: -14 .. 18)
    recs = quads(rng, n, slots, W, Hh, 16)
    counts = [2] * n
    p = FC.params(half_win=3, levels=2)
    want = FC.host_flow(L, prev, nxt, recs, counts, p)
    assert (want[1][31:] != 0).all() and len({tuple(s) for s in want[0]["square"][:, 0].tolist()}) == n
    same(device_flow(det, prev, nxt, recs, counts, p), want, "33 frames")
    det.close()


def test_in_place_and_without_status_and_errors(L, det128):
    rng = np.random.default_rng(25)
    n, slots, W, Hh = 2, 4, 96, 64
    prev, nxt = textured(rng, n, W, Hh, "rgb", (3, 2))
    recs = quads(rng, n, slots, W, Hh, 22)
    counts = [4, 2]
    p = FC.params(half_win=4, levels=2)
    want = FC.host_flow(L, prev, nxt, recs, counts, p)
    assert (want[0]["square"][0, 0] != recs["square"][0, 0]).any() and want[0][1, 2:].tobytes() == recs[1, 2:].tobytes()
    same(device_flow(det128, prev, nxt, recs, counts, p, in_place=True), want, "in place")
    same(device_flow(det128, prev, nxt, recs, counts, p, in_place=True, with_status=False, with_err=False), want, "in place, no status, no errors")
    same(device_flow(det128, prev, nxt, recs, counts, p, with_status=False), (guard_merge(want, recs, counts),) + want[1:], "no status")
    same(device_flow(det128, prev, nxt, recs, counts, p, with_err=False), (guard_merge(want, recs, counts),) + want[1:], "no errors")


def test_every_status_code(L, det128):
    s = FC.code_scene()
    W, Hh = s["W"], s["H"]
    fa = FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [s["A"]])
    fb = FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [s["B"]])
    fo = FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [s["occl"]])
    recs = FC.code_records(W)
    p = FC.params(half_win=5, levels=2)
    want = FC.host_flow(L, fa, fb, recs, [5], p)
    assert want[1][0].tolist() == [1, -1, -2, -6, -6, 0]
    same(device_flow(det128, fa, fb, recs, [5], p), (guard_merge(want, recs, [5]),) + want[1:], "codes 1 -1 -2 -6 0")
    # -3: a shift that carries corners out of the frame, at level 0 alone
    A2, B2 = FC.shifted_pair(np.random.default_rng(13), W, Hh, -3, -2)
    f2a, f2b = FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [A2]), FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [B2])
    r3 = FK.records([[2, 40, 40, 40, 40, 70, 4, 70], [20, 40, 60, 1, 60, 60, 20, 60]]).reshape(1, 2)
    p0 = FC.params(half_win=5, levels=0)
    want = FC.host_flow(L, f2a, f2b, r3, [2], p0)
    assert want[1][0].tolist() == [-3, -3] and want[2][0, 0].tolist()[0] == -1.0 and (want[2][0, 0, 1:3] >= 0).all()
    same(device_flow(det128, f2a, f2b, r3, [2], p0), want, "code -3")
    # -4 and -5 on the occluded frame: error limits around a measured error, the forward-backward check on and off
    r4 = FK.records([[40, 56, 100, 50, 100, 85, 20, 85], [75, 50, 115, 52, 113, 88, 73, 86]]).reshape(1, 2)   # corner 0 of the first under the occluder
    base = FC.host_flow(L, fa, fo, r4, [2], p)
    assert base[1][0].tolist() == [1, 1]
    e = float(base[2][0, 0].max())
    for max_err, status in ((float(np.nextafter(np.float32(e), np.float32(np.inf))), 1), (e, 1), (float(np.nextafter(np.float32(e), np.float32(0))), -4)):
        pe = FC.params(half_win=5, levels=2, max_err=max_err)
        want = FC.host_flow(L, fa, fo, r4, [2], pe)
        assert want[1][0, 0] == status
        same(device_flow(det128, fa, fo, r4, [2], pe), want, "max_err %r" % max_err)
    for fb_max, status in ((0.0, 1), (1.0, -5)):
        pf = FC.params(half_win=5, levels=2, fb_max=fb_max)
        want = FC.host_flow(L, fa, fo, r4, [2], pf)
        assert want[1][0].tolist() == [status, 1]
        same(device_flow(det128, fa, fo, r4, [2], pf), want, "fb_max %r" % fb_max)
    pf = FC.params(half_win=5, levels=2, fb_max=1.0)
    want = FC.host_flow(L, fa, fb, recs, [5], pf)
    assert want[1][0].tolist() == [1, -1, -2, -6, -6, 0]
    same(device_flow(det128, fa, fb, recs, [5], pf), (guard_merge(want, recs, [5]),) + want[1:], "fb_max on the open scene")


def set_camera(oa, det, cam):
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))


def test_the_pose_flag_takes_the_camera_of_the_call(oa, L):
    """OCVAR_FLOW_POSE with camera A, set_camera(B) right after the call, nothing waited for: the poses are camera A's"""
    import torch
    s = FC.code_scene()
    W, Hh = s["W"], s["H"]
    det = oa.Detector(W, Hh, max_batch=1)
    fa = FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [s["A"]])
    fb = FC.fill_frames(FK.Frames(1, W, Hh, "gray"), [s["B"]])
    recs = FC.code_records(W)
    cam_a, cam_b = H.oracle_camera(W, Hh), H.oracle_camera(W, Hh)
    cam_b.cameraMatrix[0] *= 1.7
    cam_b.distCoeffs[0] = -0.2
    p = FC.params(half_win=5, levels=2, flags=FC.POSE)
    want_a = FC.host_flow(L, fa, fb, recs, [5], p, cam=cam_a)
    want_b = FC.host_flow(L, fa, fb, recs, [5], p, cam=cam_b)
    assert np.abs(want_a[0]["glMatrix"][0, 0] - want_b[0]["glMatrix"][0, 0]).max() > 1e-2
    assert (want_a[0]["glMatrix"][0, 0] != recs["glMatrix"][0, 0]).any() and want_a[0][0, 1:].tobytes() == recs[0, 1:].tobytes()
    dp, dn, dm, dc = to_device(fa.buf), to_device(fb.buf), to_device(recs), to_device(np.array([5], np.int32))
    ds = to_device(np.zeros(6, np.int32))
    torch.cuda.synchronize()
    set_camera(oa, det, cam_a)
    det.flow_records(dp.data_ptr() + fa.offset(0), dn.data_ptr() + fb.offset(0), W, Hh, 1, dm.data_ptr(), dc.data_ptr(), dm.data_ptr(), per_frame=6,
                     fmt="gray", params=p, d_status_ptr=ds.data_ptr())
    set_camera(oa, det, cam_b)
    torch.cuda.synchronize()
    got = dm.cpu().numpy().view(FK.MARKER_DTYPE).reshape(1, 6)
    same((got, ds.cpu().numpy().view(np.int32).reshape(1, 6), None), want_a, "camera by value", pose=True)
    # the pose keyword of the binding sets the flag
    dm2 = to_device(recs)
    det.flow_records(dp.data_ptr() + fa.offset(0), dn.data_ptr() + fb.offset(0), W, Hh, 1, dm2.data_ptr(), dc.data_ptr(), dm2.data_ptr(), per_frame=6,
                     fmt="gray", params=FC.params(half_win=5, levels=2), pose=True)
    torch.cuda.synchronize()
    same((dm2.cpu().numpy().view(FK.MARKER_DTYPE).reshape(1, 6), None, None), want_b, "pose keyword", pose=True)
    det.close()


# ---- with detection ----------------------------------------------------------------------------------------------------------------

SENTINEL = 0.123


@pytest.fixture(scope="module")
def moving():
    cam, tpls, frames = FC.moving_marker()
    return dict(cam=cam, tpls=tpls, frames=frames)


def moving_detector(oa, mv, gate=None):
    det = oa.Detector(320, 240, max_batch=1)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in mv["tpls"]])
    set_camera(oa, det, mv["cam"])
    if gate is not None:
        det.set_gate(gate)
    return det


def corners(square):
    return sorted(map(tuple, np.asarray(square).reshape(4, 2).tolist()))


def test_a_fast_marker_keeps_its_record_with_flow(oa, moving):
    """three 320 x 240 frames of a marker that moves 30 px per frame; frame 0's record gets the score 0.123, which the tracking stage
    carries.  Plain enqueue_tracked re-decodes the marker at frame 1 (the sentinel is gone); with flow_records in front the sentinel
    survives to frame 2 and the squares are the detected ones of each frame."""
    import torch
    mv = moving
    det = moving_detector(oa, mv)
    M = det.max_markers
    d = [to_device(f) for f in mv["frames"]]
    stateless = []
    for t in range(3):
        m, c = det.detect_device(d[t].data_ptr(), 320, 240, 1)
        assert c[0] == 1
        stateless.append(m[0, 0].copy())
    assert np.abs(stateless[1]["square"] - stateless[0]["square"]).max() > 20

    def first_records():
        recs = np.zeros((1, M), FK.MARKER_DTYPE)
        recs[0, 0] = stateless[0]
        recs["score"][0, 0] = SENTINEL
        return to_device(recs), to_device(np.array([1], np.int32))

    for use_flow in (False, True):
        dm, dc = first_records()
        scores = []
        for t in (1, 2):
            if use_flow:
                det.flow_records(d[t - 1].data_ptr(), d[t].data_ptr(), 320, 240, 1, dm.data_ptr(), dc.data_ptr(), dm.data_ptr())
            det.enqueue_tracked(d[t].data_ptr(), 320, 240, 1, dm.data_ptr(), dc.data_ptr())
            det.results_to_device(dm.data_ptr(), dc.data_ptr())
            m, c = det.collect()
            torch.cuda.synchronize()
            assert c[0] == 1
            scores.append(float(m["score"][0, 0]))
            assert corners(m["square"][0, 0]) == corners(stateless[t]["square"]), (use_flow, t)
            if use_flow:
                assert m["templateId"][0, 0] == stateless[0]["templateId"] and m["markerId"][0, 0] == stateless[0]["markerId"]
        if use_flow:
            assert scores == [SENTINEL, SENTINEL]
        else:
            assert scores[0] != SENTINEL and scores[1] != SENTINEL
    det.close()


@pytest.mark.parametrize("predict", [True, False])
def test_device_stream_tracker(oa, moving, predict):
    import torch
    from opencv_ar_amd.tracking import DeviceStreamTracker
    mv = moving
    det = moving_detector(oa, mv)
    trk = DeviceStreamTracker(det, 1, 320, 240, predict=predict)
    d = [to_device(f) for f in mv["frames"]]
    m, c = trk.step(d[0])
    assert c[0] == 1
    torch.cuda.synchronize()
    first = m[0, 0].copy()
    recs = trk.recs.cpu().numpy().view(FK.MARKER_DTYPE).copy()
    recs["score"][0] = SENTINEL
    trk.recs.copy_(to_device(recs))
    torch.cuda.synchronize()
    scores = []
    for t in (1, 2):
        m, c = trk.step(d[t])
        assert c[0] == 1
        scores.append(float(m["score"][0, 0]))
        ref, _ = det.detect_device(d[t].data_ptr(), 320, 240, 1)
        assert corners(m["square"][0, 0]) == corners(ref["square"][0, 0])
    if predict:
        assert scores == [SENTINEL, SENTINEL] and m["templateId"][0, 0] == first["templateId"]
    else:
        assert SENTINEL not in scores
    trk.reset()
    m, c = trk.step(d[0])
    assert c[0] == 1 and m["score"][0, 0] == first["score"]
    det.close()


def test_beside_a_batch_in_flight_under_a_gate_and_on_two_streams(oa, L, moving):
    """a flow call on a named stream while a detection batch of the same context is in flight under a gate: both results as without
    the other; then two calls on two streams back to back, which the library orders on its workspace"""
    import torch
    mv = moving
    gate = oa.Gate(width=1)
    det = moving_detector(oa, mv, gate=gate)
    d = to_device(mv["frames"][0])
    alone, alone_counts = det.detect_device(d.data_ptr(), 320, 240, 1)
    rng = np.random.default_rng(31)
    n, slots, W, Hh = 1, 3, 320, 240
    prev, nxt = textured(rng, n, W, Hh, "bgr", (6, -4), cell=8)
    prev2, nxt2 = textured(rng, n, W, Hh, "bgr", (-5, 7), cell=8)
    recs = quads(rng, n, slots, W, Hh, 70)
    p = FC.params()
    want, want2 = FC.host_flow(L, prev, nxt, recs, [3], p), FC.host_flow(L, prev2, nxt2, recs, [3], p)
    assert (want[1][0, :2] == 1).all() and (want[0]["square"] != want2[0]["square"]).any()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dev = [to_device(x.buf) for x in (prev, nxt, prev2, nxt2)]
    dm, dc = to_device(recs), to_device(np.array([3], np.int32))
    outs = [to_device(guard_like(recs)) for _ in range(3)]
    sts = [to_device(np.zeros(3, np.int32)) for _ in range(3)]
    torch.cuda.synchronize()

    def flow(k, a, b, fa, fb, stream):
        det.flow_records(dev[a].data_ptr() + fa.offset(0), dev[b].data_ptr() + fb.offset(0), W, Hh, 1, dm.data_ptr(), dc.data_ptr(), outs[k].data_ptr(),
                         per_frame=slots, fmt="bgr", prev_row_stride=fa.row_stride, next_row_stride=fb.row_stride, d_status_ptr=sts[k].data_ptr(),
                         stream=stream.cuda_stream)

    det.enqueue_device(d.data_ptr(), 320, 240, 1)
    flow(0, 0, 1, prev, nxt, s1)
    markers, counts = det.collect()
    assert counts.tolist() == alone_counts.tolist() and markers.tobytes() == alone.tobytes()
    flow(1, 2, 3, prev2, nxt2, s1)
    flow(2, 0, 1, prev, nxt, s2)
    torch.cuda.synchronize()
    for k, w in ((0, want), (1, want2), (2, want)):
        got = (outs[k].cpu().numpy().view(FK.MARKER_DTYPE).reshape(1, slots), sts[k].cpu().numpy().view(np.int32).reshape(1, slots), None)
        same(got, w, "call %d" % k)
    assert (dev[0].cpu().numpy() == prev.buf).all() and (d.cpu().numpy().reshape(-1) == mv["frames"][0].reshape(-1)).all()
    det.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa, L):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(128, 96, max_batch=2)
    ctx = det._ctx
    W, Hh, M = 128, 96, det.max_markers
    s = FC.code_scene()
    fa = FC.fill_frames(FK.Frames(2, W, Hh, "bgr"), [s["A"], s["A"]])
    fb = FC.fill_frames(FK.Frames(2, W, Hh, "bgr"), [s["B"], s["B"]])
    recs = FK.records([FC.GOOD] * 2).reshape(2, 1)
    dp, dn, dm, dc = to_device(fa.buf), to_device(fb.buf), to_device(recs), to_device(np.array([1, 1], np.int32))
    out_h = guard_like(recs)
    do, ds, de = to_device(out_h), to_device(np.full(8, FK.GUARD, np.uint8)), to_device(np.full(32, FK.GUARD, np.uint8))
    torch.cuda.synchronize()
    pp, np_ = dp.data_ptr() + fa.offset(0), dn.data_ptr() + fb.offset(0)

    def call(**kw):
        a = dict(pp=pp, prs=3 * W, np=np_, nrs=3 * W, w=W, h=Hh, n=2, fmt=0, rp=dm.data_ptr(), cp=dc.data_ptr(), per=1, op=do.data_ptr(), par={})
        a.update(kw)
        par = None if a["par"] is None else C.byref(FC.params(**a["par"]))
        return lib.ocvar_hip_flow_records(ctx, a["pp"], a["prs"], a.get("pfs", fa.frame_stride), a["np"], a["nrs"], a.get("nfs", fb.frame_stride),
                                          a["w"], a["h"], a["n"], a["fmt"], a["rp"], a["cp"], a["per"], par, a["op"], ds.data_ptr(), de.data_ptr(), None)

    span = (2 ** 31) // (Hh - 1) + 1   # a row stride with which the rows of one frame span more than 2^31 - 1 bytes
    nan, inf = float("nan"), float("inf")
    cases = [dict(pp=None), dict(np=None), dict(rp=None), dict(cp=None), dict(op=None), dict(fmt=5), dict(fmt=-1), dict(prs=3 * W - 1),
             dict(nrs=3 * W - 1), dict(fmt=2, prs=4 * W - 1, nrs=4 * W), dict(prs=span), dict(nrs=span), dict(w=129), dict(h=97),
             dict(w=22, par=dict(half_win=10)), dict(h=22, par=dict(half_win=10)), dict(w=4, par=dict(half_win=1)), dict(n=0), dict(n=-1),
             dict(per=0), dict(per=M + 1), dict(par=dict(half_win=0)), dict(par=dict(half_win=16)), dict(par=dict(levels=-1)),
             dict(par=dict(levels=6)), dict(par=dict(max_iter=0)), dict(par=dict(max_iter=101)), dict(par=dict(flags=2)), dict(par=dict(flags=-1)),
             dict(par=dict(flags=FC.POSE))]   # (no camera is set)
    for name in ("eps", "min_eig", "max_err", "fb_max"):
        cases += [dict(par={name: -1.0}), dict(par={name: nan}), dict(par={name: inf}), dict(par={name: -inf})]
    for kw in cases:
        assert call(**kw) == E_ARG, kw
        assert lib.ocvar_hip_last_error(ctx), kw
    torch.cuda.synchronize()
    assert do.cpu().numpy().tobytes() == out_h.tobytes() and (ds.cpu().numpy() == FK.GUARD).all() and (de.cpu().numpy() == FK.GUARD).all()
    # and after all that the context still tracks: the defaults of a NULL parameter block, sides of exactly 2 half_win + 3
    assert call(par=None) == 0
    torch.cuda.synchronize()
    want = FC.host_flow(L, fa, fb, recs, [1, 1], FC.params())
    got = (do.cpu().numpy().view(FK.MARKER_DTYPE).reshape(2, 1), ds.cpu().numpy().view(np.int32).reshape(2, 1), de.cpu().numpy().view(np.float32).reshape(2, 1, 4))
    same(got, want, "defaults")
    assert call(w=23, h=23, par=dict(half_win=10)) == 0
    set_camera(oa, det, H.oracle_camera(W, Hh))
    assert call(par=dict(flags=FC.POSE)) == 0
    torch.cuda.synchronize()
    det.close()

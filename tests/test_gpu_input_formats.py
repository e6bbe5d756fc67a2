"""Frames in GRAY, RGB, BGRA and RGBA on the device path (include/ocvar_hip.h: ocvar_hip_set_input_format), against the oracle
on the BGR frame with the same colours.

The synthetic frames have equal channels, on which a B/R swap or a dropped alpha byte would go unnoticed; the colour frames here
are given unequal channels first (an offset and noise of their own per channel) and the four-channel ones random alpha bytes.
GRAY frames are a grey image g, whose BGR equivalent is (g, g, g)."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
from frame_kit import oa  # noqa: F401
from test_gpu_load import NAMES, distinct_frames, oracle_all
from test_gpu_parity import OracleFrame, check_candidates, check_markers, check_planes, make_detector

pytestmark = pytest.mark.gpu

NOT_BGR = ["gray", "rgb", "bgra", "rgba"]


def unequal(bgr, seed):
    """bgr with channels that differ: a per-channel offset and per-channel noise (markers stay detectable)"""
    r = np.random.default_rng(seed)
    img = bgr.astype(np.int32) + r.integers(-30, 31, 3) + r.integers(-6, 7, bgr.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def grey_image(bgr, seed):
    r = np.random.default_rng(seed)
    return np.clip(bgr[..., 0].astype(np.int32) + r.integers(-6, 7, bgr.shape[:2]), 0, 255).astype(np.uint8)


def as_format(bgr, fmt, seed):
    """(frame in fmt, the BGR frame with the same colours) made from a synthetic frame"""
    if fmt == "gray":
        g = grey_image(bgr, seed)
        return g, np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))
    c = unequal(bgr, seed)
    alpha = np.random.default_rng(seed + 1).integers(0, 256, c.shape[:2] + (1,), dtype=np.uint8)
    src = {"bgr": c, "rgb": c[..., ::-1], "bgra": np.concatenate([c, alpha], 2), "rgba": np.concatenate([c[..., ::-1], alpha], 2)}[fmt]
    return np.ascontiguousarray(src), c


def grey_in_place_of(src, fmt, grey):
    """what grey_in_place leaves in a frame of format fmt whose grey image is `grey`"""
    if fmt == "gray":
        return src
    out = src.copy()
    out[..., :3] = grey[..., None]
    return out


def formatted_batch(cfg, n, fmt, names=None, seed=0):
    base = [H.synth_frame(cfg, f, names)[0] for f in range(n)]
    pairs = [as_format(b, fmt, seed + 17 * f) for f, b in enumerate(base)]
    return np.stack([p[0] for p in pairs]), [p[1] for p in pairs]


_hd = {}


def hd_scene(fmt):
    """64 distinct 1080p frames in fmt and their oracle results (colour formats share one set: same BGR frames)"""
    key = "gray" if fmt == "gray" else "colour"
    if key not in _hd:
        from concurrent.futures import ThreadPoolExecutor
        cfg = H.synth_config(3)
        base = [H.synth_frame(cfg, f)[0] for f in range(64)]
        tpls, cam = H.oracle_templates(), H.oracle_camera(cfg.width, cfg.height)
        bgr = [as_format(b, "gray" if key == "gray" else "bgr", 100 + f)[1] for f, b in enumerate(base)]
        with ThreadPoolExecutor(min(32, os.cpu_count() or 1)) as ex:
            refs = list(ex.map(lambda b: OracleFrame(b, tpls, cam), bgr))
        _hd[key] = (cfg, base, refs)
    cfg, base, refs = _hd[key]
    src = np.stack([as_format(b, fmt, 100 + f)[0] for f, b in enumerate(base)])
    return cfg, src, refs


@pytest.mark.parametrize("fmt", NOT_BGR)
def test_planes_of_64_distinct_full_hd_frames_in_one_launch(oa, fmt):
    """every frame of a 64-frame 1080p launch, plane by plane (grey, binary, masks), frame quads, pre-elimination candidates,
    markers and poses"""
    import torch
    cfg, src, refs = hd_scene(fmt)
    det, tpls, cam = make_detector(oa, cfg, None, 64)
    det.set_input_format(fmt)
    d = torch.from_numpy(src).cuda()
    markers, counts = det.detect_device(d.data_ptr(), cfg.width, cfg.height, 64)
    assert counts.sum() >= 64, counts   # (the markers survive the channel offsets and noise)
    for f in range(64):
        check_planes(det, f, refs[f], where=fmt)
        check_candidates(det, f, refs[f], where=fmt)
        check_markers(f, refs[f], markers, counts, where=fmt)


@pytest.mark.parametrize("fmt", NOT_BGR)
def test_odd_panel_boundary_and_smallest_sizes(oa, fmt):
    """odd widths and heights (1921x1081, and the sizes whose last column or row begins a grey panel), and the smallest frames,
    which take the byte-wise generic path (sw < 32)"""
    for (w, h) in ((1921, 1081), (487, 365), (729, 243), (961, 541)):
        cfg = H.synth_config(3, textured=1, width=w, height=h, grid_x=max(1, w // 240), grid_y=max(1, h // 240), side_min=70, side_max=110)
        det, tpls, cam = make_detector(oa, cfg, None, 2)
        det.set_input_format(fmt)
        src, bgr = formatted_batch(cfg, 2, fmt, seed=w)
        markers, counts = det.detect_host(src.copy())
        assert counts.sum() > 0
        for f in range(2):
            ref = OracleFrame(bgr[f], tpls, cam)
            check_planes(det, f, ref, where=(fmt, w, h))
            check_candidates(det, f, ref, where=(fmt, w, h))
            check_markers(f, ref, markers, counts, where=(fmt, w, h))
    rng = np.random.default_rng(5)
    for (w, h) in ((16, 16), (31, 31)):
        cfg = H.synth_config(2, width=w, height=h)
        det, tpls, cam = make_detector(oa, cfg, ["2x2-01"], 2)
        det.set_input_format(fmt)
        noise = rng.integers(0, 256, (h, w, 3), np.uint8)
        blocks = np.kron(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4, 1), np.uint8) * 255, np.ones((4, 4, 3), np.uint8))[:h, :w]
        pairs = [as_format(np.ascontiguousarray(x), fmt, 7 + i) for i, x in enumerate((noise, blocks))]
        markers, counts = det.detect_host(np.stack([p[0] for p in pairs]))
        for f in range(2):
            ref = OracleFrame(pairs[f][1], tpls, cam)
            check_planes(det, f, ref, where=(fmt, w, h))
            check_markers(f, ref, markers, counts, where=(fmt, w, h))


@pytest.mark.parametrize("fmt", NOT_BGR)
def test_padded_rows_gapped_frames_unaligned_base_and_grey_in_place(oa, fmt):
    """rows padded by 5 bytes, frames 77 bytes apart, the base pointer at an odd address; grey_in_place leaves a GRAY buffer as
    it was, makes bytes 0..2 of every other pixel the grey value and leaves the alpha bytes and the padding untouched"""
    import torch
    cfg = H.synth_config(2, width=644, height=482)
    n, bpp = 3, FK.bpp_of(fmt)
    det, tpls, cam = make_detector(oa, cfg, ["2x2-01"], n)
    det.set_input_format(fmt)
    src, bgr = formatted_batch(cfg, n, fmt, ["2x2-01"], seed=3)
    w, h = cfg.width, cfg.height
    row_stride = bpp * w + 5
    frame_stride = row_stride * h + 77
    buf = np.full(1 + n * frame_stride, 0xA5, np.uint8)
    for f in range(n):
        rows = buf[1 + f * frame_stride: 1 + f * frame_stride + row_stride * h].reshape(h, row_stride)
        rows[:, :bpp * w] = src[f].reshape(h, bpp * w)
    before = buf.copy()
    d = torch.from_numpy(buf).cuda()
    markers, counts = det.detect_device(d.data_ptr() + 1, w, h, n, row_stride=row_stride, frame_stride=frame_stride, grey_in_place=True)
    out = d.cpu().numpy()
    if fmt == "gray":
        assert np.array_equal(out, before)
    for f in range(n):
        ref = OracleFrame(bgr[f], tpls, cam)
        check_planes(det, f, ref, where=fmt)
        check_candidates(det, f, ref, where=fmt)
        check_markers(f, ref, markers, counts, where=fmt)
        rows = out[1 + f * frame_stride: 1 + f * frame_stride + row_stride * h].reshape(h, row_stride)
        px = rows[:, :bpp * w].reshape(src[f].shape)
        assert np.array_equal(px, grey_in_place_of(src[f], fmt, ref.grey)), f
        assert (rows[:, bpp * w:] == 0xA5).all()
    assert out[0] == 0xA5 and (out[1 + (n - 1) * frame_stride + row_stride * h:] == 0xA5).all()


@pytest.mark.parametrize("fmt", NOT_BGR)
def test_4k_frame(oa, fmt):
    cfg = H.synth_config(5)
    det, tpls, cam = make_detector(oa, cfg, None, 1)
    det.set_input_format(fmt)
    src, bgr = formatted_batch(cfg, 1, fmt, seed=11)
    markers, counts = det.detect_host(src.copy())
    ref = OracleFrame(bgr[0], tpls, cam)
    check_planes(det, 0, ref, where=fmt)
    check_candidates(det, 0, ref, where=fmt)
    check_markers(0, ref, markers, counts, where=fmt)
    assert counts[0] > 0


def test_nv12_luma_plane(oa):
    """GRAY on the luma plane of NV12 frames: pitch 2048, frame_stride 2048 * 1080 * 3 / 2, random bytes in the chroma part
    and the pitch padding -- the results are the oracle's on the luma image"""
    import torch
    cfg = H.synth_config(3)
    w, h, pitch, n = cfg.width, cfg.height, 2048, 3
    fs = pitch * h * 3 // 2
    det, tpls, cam = make_detector(oa, cfg, None, n)
    det.set_input_format("gray")
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 256, n * fs, dtype=np.uint8)
    lumas = []
    for f in range(n):
        g = grey_image(H.synth_frame(cfg, f)[0], 40 + f)
        buf[f * fs: f * fs + pitch * h].reshape(h, pitch)[:, :w] = g
        lumas.append(g)
    d = torch.from_numpy(buf).cuda()
    markers, counts = det.detect_device(d.data_ptr(), w, h, n, row_stride=pitch, frame_stride=fs)
    for f in range(n):
        ref = OracleFrame(np.repeat(lumas[f][..., None], 3, axis=2), tpls, cam)
        check_planes(det, f, ref, where="nv12")
        check_candidates(det, f, ref, where="nv12")
        check_markers(f, ref, markers, counts, where="nv12")
    assert counts.sum() > 0


@pytest.mark.parametrize("fmt", NOT_BGR)
def test_entry_points(oa, fmt):
    """detect_device, detect_host from pageable and from caller-pinned memory (grey_in_place: GRAY copies nothing back), a
    tracked second call through enqueue_tracked with the first call's results_to_device block"""
    import torch
    cfg = H.synth_config(2)
    n = 4
    det, tpls, cam = make_detector(oa, cfg, None, n)
    det.set_input_format(fmt)
    src, bgr = formatted_batch(cfg, n, fmt, seed=21)
    w, h = cfg.width, cfg.height
    refs = [OracleFrame(b, tpls, cam) for b in bgr]
    d = torch.from_numpy(src).cuda()
    markers, counts = det.detect_device(d.data_ptr(), w, h, n)
    for f in range(n):
        check_markers(f, refs[f], markers, counts, where=(fmt, "device"))
    for pinned in (False, True):
        work = torch.from_numpy(src.copy()).pin_memory().numpy() if pinned else src.copy()
        markers, counts = det.detect_host(work, grey_in_place=True)
        for f in range(n):
            check_planes(det, f, refs[f], where=(fmt, "host", pinned))
            check_markers(f, refs[f], markers, counts, where=(fmt, "host", pinned))
            assert np.array_equal(work[f], grey_in_place_of(src[f], fmt, refs[f].grey)), (fmt, pinned, f)
    # step 1 stateless, its results into device memory; step 2 tracked from them (enqueue_tracked)
    d_m = torch.zeros((n, oa.MAX_MARKERS * 184), dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
    det.enqueue_device(d.data_ptr(), w, h, n)
    det.results_to_device(d_m.data_ptr(), d_c.data_ptr())
    m1, c1 = det.collect()
    torch.cuda.synchronize()
    assert np.array_equal(d_c.cpu().numpy(), c1)
    blk = d_m.cpu().numpy().view(oa.MARKER_DTYPE).reshape(n, oa.MAX_MARKERS)
    for f in range(n):
        assert blk[f, :c1[f]].tobytes() == m1[f, :c1[f]].tobytes()
    lib = det._lib
    rc = lib.ocvar_hip_enqueue_tracked(det._ctx, C.c_void_p(d.data_ptr()), w, h, FK.bpp_of(fmt) * w, FK.bpp_of(fmt) * w * h, n, 0,
                                       C.c_void_p(d_m.data_ptr()), C.c_void_p(d_c.data_ptr()), None)
    assert rc == 0, rc
    det._n = n
    m2, c2 = det.collect()
    for f in range(n):
        prev = [H.Marker.from_buffer_copy(m1[f, k].tobytes()) for k in range(c1[f])]
        ref2 = OracleFrame(bgr[f], tpls, cam, prev=prev, planes=False)
        check_markers(f, ref2, m2, c2, where=(fmt, "tracked"))


@pytest.mark.parametrize("fmt", ["gray", "bgra"])
def test_pipe_submit_collect_and_track_device(oa, fmt):
    import torch
    cfg = H.synth_config(2)
    n = 12
    w, h = cfg.width, cfg.height
    tpls, cam = H.oracle_templates(), H.oracle_camera(w, h)
    src, bgr = formatted_batch(cfg, n, fmt, seed=31)
    refs = [OracleFrame(b, tpls, cam, planes=False) for b in bgr]
    d = torch.from_numpy(src).cuda()
    fb = src[0].nbytes
    pipe = oa.Pipe(w, h, chunk_frames=4, n_contexts=3, gate_width=2)
    pipe.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    pipe.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    pipe.set_input_format(fmt)
    for k in range(3):
        assert pipe.submit(d.data_ptr() + 4 * k * fb, w, h, 4, tag=k)
    for k in range(3):
        tag, m, c = pipe.collect(4)
        assert tag == k
        for p in range(4):
            check_markers(p, refs[4 * k + p], m, c, where=(fmt, "pipe", k))
    markers, counts = pipe.detect_device(d.data_ptr(), w, h, n)
    for f in range(n):
        check_markers(f, refs[f], markers, counts, where=(fmt, "pipe detect"))
    prev = [[] for _ in range(n)]
    for step in range(3):
        markers, counts = pipe.track_device(d.data_ptr(), w, h, n, reset=(step == 0))
        for f in range(n):
            ref = OracleFrame(bgr[f], tpls, cam, prev=prev[f] or None, planes=False)
            check_markers(f, ref, markers, counts, where=(fmt, "track", step))
            prev[f] = [H.Marker.from_buffer_copy(markers[f, k].tobytes()) for k in range(min(counts[f], markers.shape[1]))]
    pipe.close()


def test_multi_detect_host_on_one_device(oa):
    path = os.path.join(oa.LIB_DIR, "libocvar_multi.so")
    if not os.path.exists(path):
        pytest.skip("libocvar_multi.so not built")
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.ocvar_multi_create.argtypes = [C.POINTER(vp), vp, i, i, i, i]
    lib.ocvar_multi_destroy.argtypes = [vp]
    lib.ocvar_multi_set_templates.argtypes = [vp, vp, i]
    lib.ocvar_multi_set_camera.argtypes = [vp, vp]
    lib.ocvar_multi_set_input_format.argtypes = [vp, i]
    lib.ocvar_multi_detect_host.argtypes = [vp, vp, i, i, i, C.c_size_t, i, vp, vp, i]
    cfg = H.synth_config(2)
    w, h, n = cfg.width, cfg.height, 3
    tpls, cam = H.oracle_templates(), H.oracle_camera(w, h)
    m = vp()
    assert lib.ocvar_multi_create(C.byref(m), None, 1, w, h, n) == 0
    try:
        assert lib.ocvar_multi_set_templates(m, tpls, len(tpls)) == 0
        assert lib.ocvar_multi_set_camera(m, C.byref(cam)) == 0
        for fmt in ("gray", "rgba"):
            assert lib.ocvar_multi_set_input_format(m, oa.INPUT_FORMATS[fmt]) == 0
            src, bgr = formatted_batch(cfg, n, fmt, seed=41)
            markers = np.zeros((n, oa.MAX_MARKERS), oa.MARKER_DTYPE)
            counts = np.zeros(n, np.int32)
            assert lib.ocvar_multi_detect_host(m, H.P(src), w, h, FK.bpp_of(fmt) * w, src[0].nbytes, n, H.P(markers), H.P(counts), oa.MAX_MARKERS) == 0
            for f in range(n):
                check_markers(f, OracleFrame(bgr[f], tpls, cam, planes=False), markers, counts, where=(fmt, "multi"))
            assert lib.ocvar_multi_detect_host(m, H.P(src), w, h, FK.bpp_of(fmt) * w - 1, src[0].nbytes, n, H.P(markers), H.P(counts), oa.MAX_MARKERS) == -2
        assert lib.ocvar_multi_set_input_format(m, 5) == -2
    finally:
        lib.ocvar_multi_destroy(m)


def test_switching_formats_between_batches(oa):
    """one context BGR -> GRAY -> BGR: its BGR results are byte for byte those of a context that never switched"""
    import torch
    cfg = H.synth_config(3)
    n = 4
    w, h = cfg.width, cfg.height
    det, tpls, cam = make_detector(oa, cfg, None, n)
    plain, _, _ = make_detector(oa, cfg, None, n)
    bgr, _ = formatted_batch(cfg, n, "bgr", seed=51)
    gray, gbgr = formatted_batch(cfg, n, "gray", seed=52)
    d_bgr, d_gray = torch.from_numpy(bgr).cuda(), torch.from_numpy(gray).cuda()
    ref_m, ref_c = plain.detect_device(d_bgr.data_ptr(), w, h, n)
    m0, c0 = det.detect_device(d_bgr.data_ptr(), w, h, n)
    det.set_input_format("gray")
    mg, cg = det.detect_device(d_gray.data_ptr(), w, h, n)
    for f in range(n):
        check_markers(f, OracleFrame(gbgr[f], tpls, cam, planes=False), mg, cg, where="gray between bgr")
    det.set_input_format("bgr")
    m1, c1 = det.detect_device(d_bgr.data_ptr(), w, h, n)
    for m, c in ((m0, c0), (m1, c1)):
        assert np.array_equal(c, ref_c) and m.tobytes() == ref_m.tobytes()
    for f in range(n):
        assert np.array_equal(det.debug_masks(f, w, h), plain.debug_masks(f, w, h))


def test_errors(oa):
    import torch
    cfg = H.synth_config(2)
    w, h = cfg.width, cfg.height
    det, tpls, cam = make_detector(oa, cfg, ["2x2-01"], 2)
    d = torch.zeros(2 * 4 * w * h, dtype=torch.uint8, device="cuda")
    for fmt in ["bgr"] + NOT_BGR:
        det.set_input_format(fmt)
        with pytest.raises(oa.OcvarError, match=r"\(-2\)"):
            det.detect_device(d.data_ptr(), w, h, 2, row_stride=FK.bpp_of(fmt) * w - 1)
        det.detect_device(d.data_ptr(), w, h, 2, row_stride=FK.bpp_of(fmt) * w)
    det.set_input_format("gray")
    with pytest.raises(ValueError):
        det.detect_host(np.zeros((2, h, w, 4), np.uint8))   # gray frames are [n, H, W]
    det.set_input_format("bgra")
    with pytest.raises(ValueError):
        det.detect_host(np.zeros((2, h, w, 3), np.uint8))
    assert det._lib.ocvar_hip_set_input_format(det._ctx, 5) == -2 and det._lib.ocvar_hip_set_input_format(det._ctx, -1) == -2
    det.enqueue_device(d.data_ptr(), w, h, 2)
    assert det._lib.ocvar_hip_set_input_format(det._ctx, 4) == -2   # a batch not yet collected
    det.collect()
    assert det._lib.ocvar_hip_set_input_format(det._ctx, 4) == 0
    pipe = oa.Pipe(w, h, chunk_frames=2, n_contexts=2, gate_width=2)
    pipe.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    pipe.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    assert pipe.submit(d.data_ptr(), w, h, 2)
    assert pipe._lib.ocvar_hip_pipe_set_input_format(pipe._p, 4) == -2   # a chunk in flight
    pipe.collect(2)
    assert pipe._lib.ocvar_hip_pipe_set_input_format(pipe._p, 4) == 0
    assert pipe._lib.ocvar_hip_pipe_set_input_format(pipe._p, 7) == -2
    pipe.close()


def test_gray_at_the_benchmark_geometry(oa):
    """bench.py's schedule in GRAY: 5 contexts sharing Gate(2), 1638-frame launches (the first ones ragged), every frame's count
    and marker records against the oracle, the last launch's candidates"""
    import torch
    NS, GATE, launch, U, SHIFT = 5, 2, 1638, 64, 7
    w, h = 1920, 1080
    colour = distinct_frames(w, h, U, seed=3000)
    base = np.ascontiguousarray(colour[..., 1])
    tpls, cam = H.oracle_templates(NAMES), H.oracle_camera(w, h)
    refs = oracle_all(np.ascontiguousarray(np.repeat(base[..., None], 3, axis=3)), tpls, cam, planes=False)
    first = [max(1, ((i + 1) * launch) // NS) for i in range(NS)]
    n_dev = max(first) + launch + SHIFT * (NS - 1)
    d_base = torch.from_numpy(base).cuda()
    d = d_base[torch.arange(n_dev, device="cuda") % U].contiguous()
    torch.cuda.synchronize()
    fb = w * h
    gate = oa.Gate(GATE)
    dets = []
    for i in range(NS):
        det = oa.Detector(w, h, max_batch=launch)
        det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
        det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
        det.set_gate(gate)
        det.set_result_limit(8)
        det.set_input_format("gray")
        dets.append(det)
    for i in range(NS):
        dets[i].enqueue_device(d.data_ptr() + SHIFT * i * fb, w, h, first[i])
    got = []
    for i in range(NS):
        got.append([dets[i].collect(8)])
        dets[i].enqueue_device(d.data_ptr() + (SHIFT * i + first[i]) * fb, w, h, launch)
    for i in range(NS):
        got[i].append(dets[i].collect(8))
    n_markers = 0
    for i in range(NS):
        for L, start in enumerate((0, first[i])):
            m, c = got[i][L]
            assert len(c) == (first[i] if L == 0 else launch)
            for p in range(len(c)):
                ref = refs[(start + p + SHIFT * i) % U]
                check_markers(p, ref, m, c, where=f"gray context {i} launch {L} position {p}")
                n_markers += len(ref.markers)
        for p in range(launch):
            check_candidates(dets[i], p, refs[(first[i] + p + SHIFT * i) % U], where=f"gray context {i} launch 1 position {p}")
    assert n_markers >= sum(first) + NS * launch
    del dets, det, gate, d, d_base
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

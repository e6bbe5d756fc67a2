"""Sub-pixel corner refinement on the device (ocvar_hip_set_corner_refine) against the CPU chain of tests/refine_chain.py: the
oracle's registration, the host build of refine_core.h on every output square, the oracle's pose of the refined square.
Squares bit-exact, poses within the 1e-4 bar, everything else as without refinement."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers as H
import refine_chain as RC
from frame_kit import oa  # noqa: F401
from hostbuild import host_driver

pytestmark = pytest.mark.gpu

SET5, SET15 = (5, 30, 0.1), (15, 30, 0.1)
N = 64


@pytest.fixture(scope="module")
def L():
    return RC.build_emul()


@pytest.fixture(scope="module")
def scene():
    """64 config-3 frames (1080p), templates, camera, and the oracle's unrefined records and grey image of each"""
    cfg = H.synth_config(3)
    frames = np.stack([H.synth_frame(cfg, f)[0] for f in range(N)])
    tpls, cam = H.oracle_templates(), H.oracle_camera(cfg.width, cfg.height)
    with ThreadPoolExecutor(16) as ex:
        regs = list(ex.map(lambda f: H.oracle_registration(frames[f], tpls, cam), range(N)))
    return dict(cfg=cfg, frames=frames, tpls=tpls, cam=cam, ref=[r[0] for r in regs],
                gray=[np.ascontiguousarray(r[2][:, :, 0]) for r in regs])


def expected(L, scene, f, setting):
    return RC.refined_markers(L, scene["ref"][f], scene["gray"][f], scene["cam"], setting)


def configure(oa, det, scene):
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in scene["tpls"]])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(scene["cam"])))
    return det


def device_frames(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames)).to("cuda:0")


def run(det, d, n, W=1920, H_=1080):
    return det.detect_device(d.data_ptr(), W, H_, n)


@pytest.mark.parametrize("setting", [SET5, SET15])
def test_batch_of_64_frames(oa, L, scene, setting):
    det = configure(oa, oa.Detector(1920, 1080, max_batch=N), scene)
    det.set_corner_refine(*setting)
    d = device_frames(scene["frames"])
    markers, counts = run(det, d, N)
    moved = 0
    for f in range(N):
        exp = expected(L, scene, f, setting)
        RC.check(markers, counts, f, exp, ("batch", setting))
        moved += sum(int(not np.array_equal(np.array(e.square, np.float32), np.array(r.square, np.float32)))
                     for e, r in zip(exp, scene["ref"][f]))
    assert moved > N   # the refinement did move corners


def test_off_means_off(oa, L, scene):
    d = device_frames(scene["frames"][:16])
    plain = configure(oa, oa.Detector(1920, 1080, max_batch=16), scene)
    m0, c0 = run(plain, d, 16)
    det = configure(oa, oa.Detector(1920, 1080, max_batch=16), scene)
    det.set_corner_refine(*SET5)
    m1, c1 = run(det, d, 16)
    det.set_corner_refine(half_win=0)
    m2, c2 = run(det, d, 16)
    assert np.array_equal(c0, c2) and m0.tobytes() == m2.tobytes()
    assert np.array_equal(c0, c1) and m0.tobytes() != m1.tobytes()
    for f in range(16):
        ref = scene["ref"][f]
        for k, r in enumerate(ref):   # unrefined: the oracle's squares
            assert np.array_equal(m0[f, k]["square"], np.array(r.square, np.float32))


def test_setter_ranges(oa):
    det = oa.Detector(640, 480, max_batch=1)
    lib = oa.hip_lib()
    for args in ((-1, 30, 0.1), (16, 30, 0.1), (5, 0, 0.1), (5, 101, 0.1), (5, 30, -1.0), (5, 30, float("nan"))):
        assert lib.ocvar_hip_set_corner_refine(det._ctx, *args) == -2, args
    for args in ((0, 1, 0.0), (1, 1, 0.0), (15, 100, 5.0)):
        assert lib.ocvar_hip_set_corner_refine(det._ctx, *args) == 0, args
    with pytest.raises(ValueError):
        det.set_corner_refine(16)


def tracked_expectation(L, scene, order, setting):
    """3 steps over streams: stream s sees frames order[t][s]; each step's refined records are the next step's prev"""
    prev = [None] * len(order[0])
    steps = []
    for t, fr in enumerate(order):
        out = []
        for s, f in enumerate(fr):
            exp, _ = RC.expected(L, scene["frames"][f], scene["tpls"], scene["cam"], setting, prev=prev[s])
            out.append(exp)
        prev = out
        steps.append(out)
    return steps


# static streams (tracked markers) and scene changes.  In these scenes a refined and an unrefined prev lead to the same
# association (corners move by < 2 px, markers by far less than 20 px between steps): this test checks the refined squares of
# every step and that the chain carries them, test_tracking_compares_the_callers_refined_squares below that the 20-px rule
# really compares them.
ORDER = [[0, 1, 2, 3], [0, 1, 2, 3], [4, 1, 5, 3]]


def test_tracked_steps(oa, L, scene):
    import torch
    S = len(ORDER[0])
    steps = tracked_expectation(L, scene, ORDER, SET5)
    det = configure(oa, oa.Detector(1920, 1080, max_batch=S), scene)
    det.set_corner_refine(*SET5)
    M = det.max_markers
    d_prev = torch.zeros((S, M, oa.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    pipe = oa.Pipe(1920, 1080, chunk_frames=2, n_contexts=2, gate_width=2)
    pipe.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in scene["tpls"]])
    pipe.set_camera(oa.Camera.from_buffer_copy(bytes(scene["cam"])))
    pipe.set_corner_refine(*SET5)
    for t, fr in enumerate(ORDER):
        d = device_frames(scene["frames"][fr])
        det.enqueue_tracked(d.data_ptr(), 1920, 1080, S, d_prev.data_ptr(), d_cnt.data_ptr())
        m, c = det.collect()
        pm, pc = pipe.track_device(d.data_ptr(), 1920, 1080, S, reset=(t == 0))
        for s in range(S):
            RC.check(m, c, s, steps[t][s], ("enqueue_tracked", t))
            RC.check(pm, pc, s, steps[t][s], ("pipe.track_device", t))
        d_prev.copy_(torch.from_numpy(m.view(np.uint8).reshape(S, M, -1)).to("cuda:0"))
        d_cnt.copy_(torch.from_numpy(np.minimum(c, M).astype(np.int32)).to("cuda:0"))
    assert any(len(steps[1][s]) > 0 for s in range(S))


def marker_row(oa, m):
    return np.frombuffer(bytes(m), oa.MARKER_DTYPE)[0]


def test_tracking_compares_the_callers_refined_squares(oa, L, scene):
    """prev markers at the 20-px boundary (refine_chain.moved_prev): moved so that the refined record is not tracked where the
    unrefined one would be.  The device, given the refined records as prev (host and device-resident), gives the chain of the
    refined records, which differs from that of the unrefined ones."""
    import torch
    frames = [0, 1, 2, 3]
    S = len(frames)
    prevs, exp = [], []
    for f in frames:
        pr, pu = RC.moved_prev(expected(L, scene, f, SET5), scene["ref"][f])
        assert pr
        er, _ = RC.expected(L, scene["frames"][f], scene["tpls"], scene["cam"], SET5, prev=pr)
        eu, _ = RC.expected(L, scene["frames"][f], scene["tpls"], scene["cam"], SET5, prev=pu)
        assert RC.records_differ(er, eu)   # the case can tell the two apart
        prevs.append(pr)
        exp.append(er)
    det = configure(oa, oa.Detector(1920, 1080, max_batch=S), scene)
    det.set_corner_refine(*SET5)
    d = device_frames(scene["frames"][frames])
    m, c = det.detect_device(d.data_ptr(), 1920, 1080, S, prev=[[marker_row(oa, x) for x in p] for p in prevs])
    M = det.max_markers
    pm = np.zeros((S, M), oa.MARKER_DTYPE)
    for s_, p in enumerate(prevs):
        for k, x in enumerate(p):
            pm[s_, k] = marker_row(oa, x)
    d_prev = torch.from_numpy(pm.view(np.uint8).reshape(S, -1)).to("cuda:0")
    d_cnt = torch.tensor([len(p) for p in prevs], dtype=torch.int32, device="cuda:0")
    det.enqueue_tracked(d.data_ptr(), 1920, 1080, S, d_prev.data_ptr(), d_cnt.data_ptr())
    m2, c2 = det.collect()
    for s_ in range(S):
        RC.check(m, c, s_, exp[s_], ("boundary, host prev", s_))
        RC.check(m2, c2, s_, exp[s_], ("boundary, device prev", s_))


def test_dense_frames_with_more_jobs_than_the_grid(oa, L):
    """16 frames of tests/dense_synth.py with 312 markers each on a dense context: 4992 marker records, more than the kernel's
    grid of 4096 waves, so waves take a second marker.  Every refined square equals the host core's refinement of the same
    context's unrefined square, on the frame's grey image; ids, templates and scores are those of the unrefined run; poses are
    the oracle's pose of the refined square within the bar."""
    import dense_synth as D
    n_markers, n = 24 * 13, 16
    names = D.library(n_markers)
    cfg = D.config(1920, 1080, 24, 13)
    distinct = [D.frame(cfg, i, names) for i in range(4)]
    frames = np.stack([distinct[i % 4] for i in range(n)])
    assert all(np.array_equal(f[..., 0], f[..., c]) for f in distinct for c in (1, 2))   # grey image = channel 0
    tpls, cam = H.oracle_templates(names), H.oracle_camera(1920, 1080)
    det = oa.Detector(1920, 1080, max_batch=n, max_quads=1024, max_markers=512)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    d = device_frames(frames)
    m0, c0 = run(det, d, n)
    det.set_corner_refine(*SET5)
    m1, c1 = run(det, d, n)
    assert c0.sum() > 4096 and np.array_equal(c0, c1)
    moved = 0
    for f in range(n):
        gray = np.ascontiguousarray(distinct[f % 4][..., 0])
        k = int(c0[f])
        assert k <= m0.shape[1]
        a, b = m0[f, :k], m1[f, :k]
        assert np.array_equal(a["templateId"], b["templateId"]) and np.array_equal(a["markerId"], b["markerId"])
        assert np.array_equal(a["score"], b["score"]) and np.array_equal(a["aspectRatio"], b["aspectRatio"])
        want = RC.refine_points(L, gray, a["square"].reshape(-1, 2), *SET5).reshape(k, 8)
        assert np.array_equal(b["square"], want), ("square", f, np.argwhere(b["square"] != want)[:4].tolist())
        moved += int((want != a["square"]).any(axis=1).sum())
        for j in range(k):
            sq = np.ascontiguousarray(want[j])
            gl = np.zeros(16, np.float64)
            H.oracle().orc_square_to_matrix(H.P(sq), C.byref(cam), C.c_double(float(b["aspectRatio"][j])), H.P(gl))
            assert np.abs(b["glMatrix"][j] - gl).max() <= RC.POSE_RTOL * max(1.0, np.abs(gl).max()), ("pose", f, j)
    assert moved > c0.sum() // 2


def test_dense_context(oa, L, scene):
    det = configure(oa, oa.Detector(1920, 1080, max_batch=8, max_quads=1024, max_markers=512), scene)
    det.set_corner_refine(*SET5)
    d = device_frames(scene["frames"][:8])
    markers, counts = run(det, d, 8)
    for f in range(8):
        RC.check(markers, counts, f, expected(L, scene, f, SET5), "dense")


def test_pipe_submit_collect(oa, L, scene):
    pipe = oa.Pipe(1920, 1080, chunk_frames=16, n_contexts=5, gate_width=2)
    pipe.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in scene["tpls"]])
    pipe.set_camera(oa.Camera.from_buffer_copy(bytes(scene["cam"])))
    pipe.set_corner_refine(*SET5)
    d = device_frames(scene["frames"])
    for k in range(4):
        assert pipe.submit(d[16 * k].data_ptr(), 1920, 1080, 16, tag=k)
    with pytest.raises(oa.OcvarError):
        pipe.set_corner_refine(*SET15)
    assert oa.hip_lib().ocvar_hip_pipe_set_corner_refine(pipe._p, 5, 30, 0.1) == -2
    seen = set()
    while True:
        got = pipe.collect(16)
        if got is None:
            break
        tag, markers, counts = got
        seen.add(tag)
        for f in range(16):
            RC.check(markers, counts, f, expected(L, scene, 16 * tag + f, SET5), ("pipe", tag))
    assert seen == {0, 1, 2, 3}
    pipe.set_corner_refine(half_win=0)   # nothing in flight: accepted


@pytest.mark.parametrize("fmt", ["gray", "rgba"])
def test_input_formats_give_the_bgr_result(oa, L, scene, fmt):
    n = 8
    bgr = scene["frames"][:n]
    if fmt == "gray":
        src = np.ascontiguousarray(bgr[..., 0])
        assert all(np.array_equal(bgr[..., 0], bgr[..., c]) for c in (1, 2))   # (synthetic frames: equal channels)
    else:
        alpha = np.random.default_rng(5).integers(0, 256, bgr.shape[:3] + (1,), dtype=np.uint8)
        src = np.ascontiguousarray(np.concatenate([bgr[..., ::-1], alpha], 3))
    ref = configure(oa, oa.Detector(1920, 1080, max_batch=n), scene)
    ref.set_corner_refine(*SET5)
    m0, c0 = run(ref, device_frames(bgr), n)
    det = configure(oa, oa.Detector(1920, 1080, max_batch=n), scene)
    det.set_corner_refine(*SET5)
    det.set_input_format(fmt)
    m1, c1 = run(det, device_frames(src), n)
    assert np.array_equal(c0, c1) and m0.tobytes() == m1.tobytes()
    for f in range(n):
        RC.check(m1, c1, f, expected(L, scene, f, SET5), fmt)


def test_host_mirror_registration(oa, L, scene, tmp_path):
    exe = host_driver("refine_registration_driver")
    order = [0, 0, 4]   # a static step (tracked markers), then a new scene
    tpls, cam = scene["tpls"], scene["cam"]
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array([1920, 1080, len(tpls), len(order)], np.int32).tobytes() + bytes(tpls) + bytes(cam)
                    + b"".join(scene["frames"][f].tobytes() for f in order))
    r = subprocess.run([exe, str(inp), str(out), "5", "30", "0.1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw, pos, prev = out.read_bytes(), 0, None
    size = oa.MARKER_DTYPE.itemsize
    for t, f in enumerate(order):
        count, n_out = np.frombuffer(raw[pos:pos + 8], np.int32)
        pos += 8
        markers = np.frombuffer(raw[pos:pos + n_out * size], oa.MARKER_DTYPE)
        pos += n_out * size
        exp, _ = RC.expected(L, scene["frames"][f], tpls, cam, SET5, prev=prev)
        RC.check(markers[None, :], np.array([count]), 0, exp, ("cvarArMultRegistration", t))
        prev = exp
    assert pos == len(raw)


def test_accuracy_on_the_device(oa, scene):
    """the CPU accuracy property (tests/test_corner_refine_cpu.py) on the device's own output"""
    n = 24
    d = device_frames(scene["frames"][:n])
    plain = configure(oa, oa.Detector(1920, 1080, max_batch=n), scene)
    m0, c0 = run(plain, d, n)
    det = configure(oa, oa.Detector(1920, 1080, max_batch=n), scene)
    det.set_corner_refine(*SET5)
    m1, c1 = run(det, d, n)
    e0, e1 = [], []
    for f in range(n):
        truth = H.synth_frame(scene["cfg"], f)[1]
        e0.append(RC.corner_errors([m0[f, k]["square"] for k in range(c0[f])], truth))
        e1.append(RC.corner_errors([m1[f, k]["square"] for k in range(c1[f])], truth))
    e0, e1 = np.concatenate(e0), np.concatenate(e1)
    assert len(e0) == len(e1) >= 100
    assert np.median(e1) <= 0.3 and np.percentile(e1, 95) <= 0.5, (np.median(e1), np.percentile(e1, 95))
    assert np.median(e1) < 0.5 * np.median(e0) and np.percentile(e1, 95) < 0.5 * np.percentile(e0, 95)

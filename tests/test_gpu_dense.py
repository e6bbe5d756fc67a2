"""GPU tests of dense contexts (ocvar_hip_create_dense: up to 16384 squares and 4096 markers per frame) against the oracle: a
4K grid of thousands of squares through cvarFindSquares and ocvar_hip_find_squares, 16-frame batches of 4K frames with more
than 1792 squares and more than 1000 markers, of 1080p frames with hundreds of markers, tracking with more than 64 markers
carried in (detect_host, enqueue_tracked, cvarArMultRegistration of libopencv-ar.so), and the result strides.  Every frame here
fails on a default context; that is checked too."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dense_synth as D
import helpers as H
from frame_kit import oa  # noqa: F401
from hostbuild import host_core, host_driver

pytestmark = pytest.mark.gpu

LIB = os.path.join(H.PKG, "lib", "libopencv-ar.so.1.0.0")


@pytest.fixture(scope="module")
def emul():
    """host build of the tracking cores (tests/emul/dense_emul.cpp): how many markers the literal loop tracks"""
    L = host_core("dense_emul")
    L.dense_track_literal.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return L


def n_tracked(emul, prev, frame):
    """markers of `prev` the reference's tracking loop takes squares for in this (grey) frame: its reserve count"""
    sq = np.ascontiguousarray(D.oracle_squares(frame[:, :, 0]).reshape(-1, 8).astype(np.float32))
    m = (H.Marker * len(prev))()
    for i, p in enumerate(prev):
        m[i] = p
    res = np.zeros(len(prev) * 2 + 1, np.int32)
    nr = C.c_int(0)
    emul.dense_track_literal(m, len(prev), H.P(sq), len(sq), H.P(res), len(res), C.byref(nr))
    return nr.value


def marker_rows(oa, ms):
    rows = np.zeros(len(ms), oa.MARKER_DTYPE)
    for k, m in enumerate(ms):
        rows[k] = np.frombuffer(bytes(m), oa.MARKER_DTYPE)[0]
    return rows


def grid_of_squares(w, h, pitch=40, side=28):
    g = np.full((h, w), 200, np.uint8)
    for y in range(20, h - side - 20, pitch):
        for x in range(20, w - side - 20, pitch):
            g[y:y + side, x:x + side] = 40
    return g


def test_4k_grid_of_squares_through_find_squares(oa):
    """~5000 squares in one 4K image: past every rung of ocvar_hip_create_ex.  cvarFindSquares of libopencv-ar.so (its retry
    ladder now climbs to dense contexts) and ocvar_hip_find_squares on a dense context give the oracle's sequence, in order."""
    from test_gpu_boundary import CvSeq, ipl, seq_points
    g = grid_of_squares(3840, 2160)
    ref = D.oracle_squares(g)
    assert len(ref) > 4096
    host = C.CDLL(LIB)
    host.cvarFindSquares.restype = C.POINTER(CvSeq)
    host.cvarFindSquares.argtypes = [C.c_void_p, C.c_void_p]
    img_arr = np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
    img = ipl(img_arr)
    seq = host.cvarFindSquares(C.byref(img), None)
    assert seq.contents.total == 4 * len(ref)
    assert np.array_equal(seq_points(seq), ref)
    det = oa.Detector(3840, 2160, max_batch=1, max_quads=16384, max_markers=64)
    assert det.max_markers == 64 and det.max_quads == 16384
    quads, n = det.find_squares(g)
    assert n == len(ref)
    assert np.array_equal(quads, ref)


N_MARKERS = 24 * 13   # 1080p grid of 50 px markers, one template each


@pytest.fixture(scope="module")
def scene():
    """two 1080p frames with 312 markers each, and the oracle's registration of each (markers and candidates)"""
    names = D.library(N_MARKERS)
    cfg = D.config(1920, 1080, 24, 13)
    frames = [D.frame(cfg, i, names) for i in range(2)]
    tpls, cam = H.oracle_templates(names), H.oracle_camera(1920, 1080)
    with ThreadPoolExecutor(2) as ex:
        refs = list(ex.map(lambda f: H.oracle_registration(f, tpls, cam, max_markers=8192, max_cands=400000)[:2], frames))
    for m, c in refs:
        assert 64 < len(m) < 8192 and len(c) < 400000
    return dict(names=names, cfg=cfg, frames=frames, tpls=tpls, cam=cam, refs=refs)


def configured(oa, det, scene):
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in scene["tpls"]])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(scene["cam"])))
    return det


def check_markers(markers, count, ref, what):
    assert count == len(ref), (what, count, len(ref))
    for k, r in enumerate(ref):
        m = markers[k]
        assert m["templateId"] == r.templateId and m["markerId"] == r.markerId, (what, k)
        assert np.abs(m["square"] - np.array(r.square)).max() <= 0.5, (what, k)
        g = np.array(r.glMatrix)
        assert np.abs(m["glMatrix"] - g).max() <= 1e-4 * max(1.0, np.abs(g).max()), (what, k)


def test_dense_batch_of_16_frames_with_hundreds_of_markers(oa, scene):
    import torch
    ref_sq = D.oracle_squares(scene["frames"][0][:, :, 0])
    assert len(ref_sq) > 256   # (past a default context's squares as well as its markers)
    batch = np.stack([scene["frames"][i % 2] for i in range(16)])
    det = configured(oa, oa.Detector(1920, 1080, max_batch=16, max_quads=1024, max_markers=512), scene)
    assert det.max_markers == 512
    d = torch.from_numpy(batch).cuda()
    torch.cuda.synchronize()
    markers, counts = det.detect_device(d.data_ptr(), 1920, 1080, 16)
    assert markers.shape == (16, 512)
    assert oa.hip_lib().ocvar_hip_capacity_flags(det._ctx) == 0
    for f in range(16):
        check_markers(markers[f], counts[f], scene["refs"][f % 2][0], ("frame", f))
    for f in range(2):   # the pre-elimination list
        got, ref = det.debug_candidates(f), scene["refs"][f][1]
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert (a.markerId, a.templateId, a.orient, a.bit) == (b.markerId, b.templateId, b.orient, b.bit)
            assert np.abs(np.array(a.square) - np.array(b.square)).max() <= 0.5
    # the same frame on a default context: loud failure (flag 128: more than 64 markers; 4: more than 256 squares)
    small = configured(oa, oa.Detector(1920, 1080, max_batch=1), scene)
    with pytest.raises(oa.OcvarError):
        small.detect_host(scene["frames"][0][None].copy())
    assert oa.hip_lib().ocvar_hip_capacity_flags(small._ctx) & (128 | 4)


def test_dense_result_strides(oa, scene):
    import torch
    det = configured(oa, oa.Detector(1920, 1080, max_batch=2, max_quads=1024, max_markers=512), scene)
    d = torch.from_numpy(np.stack(scene["frames"])).cuda()
    torch.cuda.synchronize()
    k = 40
    det.set_result_limit(k)
    markers, counts = det.detect_device(d.data_ptr(), 1920, 1080, 2, max_per_frame=k)
    for f in range(2):
        ref = scene["refs"][f][0]
        assert counts[f] == len(ref) > k
        check_markers(markers[f], k, ref[:k], ("limit", f))
    with pytest.raises(oa.OcvarError):
        det.set_result_limit(513)
    det.set_result_limit(512)
    det.enqueue_device(d.data_ptr(), 1920, 1080, 2)
    dm = torch.zeros((2, k, oa.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    dc = torch.zeros(2, dtype=torch.int32, device="cuda")
    det.results_to_device(dm.data_ptr(), dc.data_ptr(), per_frame=k)
    full, _ = det.collect()
    torch.cuda.synchronize()
    got = dm.cpu().numpy().view(oa.MARKER_DTYPE).reshape(2, k)
    assert dc.cpu().tolist() == [len(r[0]) for r in scene["refs"]]
    for f in range(2):
        assert got[f].tobytes() == full[f, :k].tobytes()


@pytest.fixture(scope="module")
def chain(scene, emul):
    """three steps of a stream (frames 1, 0, 1) after frame 0's stateless result: the oracle's registration of each step with
    the previous step's markers carried in, and how many of them the tracking loop took squares for"""
    steps, prev = [], list(scene["refs"][0][0])
    for fi in [1, 0, 1]:
        frame = scene["frames"][fi]
        ref, _, _ = H.oracle_registration(frame, scene["tpls"], scene["cam"], prev=prev, max_markers=8192, max_cands=1)
        assert 64 < len(ref) < 8192
        tracked = n_tracked(emul, prev, frame)
        assert tracked > 64   # (the replay's matches and skips are exercised, with more markers than a default context holds)
        steps.append(dict(fi=fi, prev=prev, ref=ref, tracked=tracked))
        prev = ref
    return steps


def test_tracking_with_hundreds_of_markers_carried_in(oa, scene, chain):
    """detect_host(prev=...) and enqueue_tracked (prev in device memory) against the oracle's registration with n_in markers"""
    import torch
    det = configured(oa, oa.Detector(1920, 1080, max_batch=1, max_quads=1024, max_markers=4096), scene)
    dev = configured(oa, oa.Detector(1920, 1080, max_batch=1, max_quads=1024, max_markers=4096), scene)
    M = det.max_markers
    for t, st in enumerate(chain):
        frame, prev, ref = scene["frames"][st["fi"]], st["prev"], st["ref"]
        rows = marker_rows(oa, prev)
        markers, counts = det.detect_host(np.ascontiguousarray(frame[None]), prev=[list(rows)])
        check_markers(markers[0], counts[0], ref, ("detect_host", t))
        pm = np.zeros((1, M), oa.MARKER_DTYPE)
        pm[0, :len(prev)] = rows
        d_prev = torch.from_numpy(pm.view(np.uint8)).cuda()
        d_cnt = torch.tensor([len(prev)], dtype=torch.int32, device="cuda")
        d_frame = torch.from_numpy(np.ascontiguousarray(frame[None])).cuda()
        torch.cuda.synchronize()
        dev.enqueue_tracked(d_frame.data_ptr(), 1920, 1080, 1, d_prev.data_ptr(), d_cnt.data_ptr())
        m2, c2 = dev.collect()
        check_markers(m2[0], c2[0], ref, ("enqueue_tracked", t))


def run_tracking_driver(oa, tmp_path, scene, initial, frame_ids, tag):
    exe = host_driver("tracking_driver")
    inp, out = tmp_path / f"in_{tag}.bin", tmp_path / f"out_{tag}.bin"
    tpls = scene["tpls"]
    inp.write_bytes(np.array([1920, 1080, len(tpls), len(frame_ids), len(initial)], np.int32).tobytes() + bytes(tpls) +
                    bytes(scene["cam"]) + b"".join(bytes(m) for m in initial) +
                    b"".join(scene["frames"][i].tobytes() for i in frame_ids))
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw, off, steps = out.read_bytes(), 0, []
    for _ in frame_ids:
        count, n_out = np.frombuffer(raw[off:off + 8], np.int32)
        off += 8
        steps.append((int(count), np.frombuffer(raw[off:off + n_out * oa.MARKER_DTYPE.itemsize], oa.MARKER_DTYPE)))
        off += n_out * oa.MARKER_DTYPE.itemsize
    return steps


def test_host_mirror_tracking_with_hundreds_of_markers(oa, scene, chain, tmp_path):
    """cvarArMultRegistration with the `markers` vector carried across calls, each run in a fresh process (a fresh default
    context).  A: the stream starts empty -- the first frame has > 64 markers and > 256 squares, fails on the default context
    with flags 128 | 4 and is run again on a dense one.  B: the stream starts with > 64 markers carried in, which picks a
    context whose marker stride holds them.  Every step equals the oracle's registration."""
    a = run_tracking_driver(oa, tmp_path, scene, [], [0] + [st["fi"] for st in chain], "a")
    check_markers(a[0][1], a[0][0], scene["refs"][0][0], ("A", 0))
    for t, st in enumerate(chain):
        check_markers(a[t + 1][1], a[t + 1][0], st["ref"], ("A", t + 1))
    b = run_tracking_driver(oa, tmp_path, scene, list(scene["refs"][0][0]), [st["fi"] for st in chain], "b")
    for t, st in enumerate(chain):
        check_markers(b[t][1], b[t][0], st["ref"], ("B", t))


def test_4k_batch_with_thousands_of_squares_and_markers(oa):
    """16 frames of 3840 x 2160 with a 64 x 36 grid of small markers: more than 1792 frame-pass squares (past ocvar_hip_create_ex,
    and more than one sorted chunk of the ordering) and, every square carried in as a previous marker, more than 1000 markers per
    frame (the tracked ones bypass the elimination, as in the reference).  Counts, ids, squares, poses and the pre-elimination
    list equal the oracle's; no capacity flag is set.  A default context fails on the same frames."""
    import torch
    names = D.library(3)
    cfg = D.config(3840, 2160, 64, 36, side=30)
    frames = [D.frame(cfg, i, names) for i in range(2)]
    tpls, cam = H.oracle_templates(names), H.oracle_camera(3840, 2160)
    prevs, refs = [], []
    for f in frames:
        sq = D.oracle_squares(f[:, :, 0])
        assert len(sq) > 1792
        prev = (H.Marker * len(sq))()
        for i, q in enumerate(sq):
            prev[i].square[:] = [float(v) for v in q.reshape(-1)]
            prev[i].templateId, prev[i].markerId, prev[i].score, prev[i].aspectRatio = i % 3, i, 1.0, 1.0
        prevs.append(list(prev))
    with ThreadPoolExecutor(2) as ex:
        refs = list(ex.map(lambda k: H.oracle_registration(frames[k], tpls, cam, prev=prevs[k], max_markers=8192, max_cands=200000)[:2],
                           range(2)))
    for m, c in refs:
        assert 1000 < len(m) < 4096 and len(c) < 200000
    det = oa.Detector(3840, 2160, max_batch=16, max_quads=16384, max_markers=4096)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    d = torch.from_numpy(np.stack([frames[i % 2] for i in range(16)])).cuda()
    torch.cuda.synchronize()
    markers, counts = det.detect_device(d.data_ptr(), 3840, 2160, 16, prev=[list(marker_rows(oa, prevs[i % 2])) for i in range(16)])
    assert oa.hip_lib().ocvar_hip_capacity_flags(det._ctx) == 0
    for f in range(16):
        check_markers(markers[f], counts[f], refs[f % 2][0], ("4k", f))
    for f in range(2):
        got, ref = det.debug_candidates(f), refs[f][1]
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert (a.markerId, a.templateId, a.orient, a.bit) == (b.markerId, b.templateId, b.orient, b.bit)
    small = oa.Detector(3840, 2160, max_batch=1)
    small.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    small.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    with pytest.raises(oa.OcvarError):
        small.detect_host(np.ascontiguousarray(frames[0][None]), prev=[list(marker_rows(oa, prevs[0]))[:64]])
    assert oa.hip_lib().ocvar_hip_capacity_flags(small._ctx) & 4

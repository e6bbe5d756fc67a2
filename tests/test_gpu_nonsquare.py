"""Templates with width != height on the device path (tests/nonsquare_scenes.py) against the oracle: decode_kernel's
per-size-class patches and lane-to-cell map, finalise_kernel's aspectRatio, pose_kernel at ratio != 1, the tracked path that
carries aspectRatio in prev, corner refinement, dense contexts, Pipe, cvarArMultRegistration of libopencv-ar.so, and the host
expansion of ocvar_hip_debug_candidates.

Ids, scores, squares, ratios and candidates are bit-exact on every record; glMatrix is within 1e-4 on every record whose pose
the reference itself defines (nonsquare_scenes.pose_is_defined; tests/test_nonsquare_cpu.py counts the exclusions)."""
import numpy as np
import pytest

import helpers as H
import nonsquare_scenes as NS
from frame_kit import oa  # noqa: F401
from hostbuild import host_driver

pytestmark = pytest.mark.gpu

POSE_RTOL = NS.POSE_RTOL
CAND = np.dtype(H.Candidate)
CAND_FIELDS = ["markerId", "templateId", "orient", "bit", "square", "patPoint"]


def detector(oa, which, cam, batch=16, **kw):
    det = oa.Detector(NS.WIDTH, NS.HEIGHT, max_batch=batch, **kw)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in NS.library(which)[1]])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    return det


def device_frames(scenes):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(np.stack([s.frame for s in scenes]))).to("cuda:0")
    torch.cuda.synchronize()
    return d


def check_candidates(cands, ref, where):
    assert len(cands) == len(ref), ("candidate count", where, len(cands), len(ref))
    a = np.frombuffer(b"".join(bytes(c) for c in cands), CAND)[CAND_FIELDS]
    b = np.frombuffer(b"".join(bytes(c) for c in ref), CAND)[CAND_FIELDS]
    if not np.array_equal(a, b):
        k = int(np.flatnonzero(a != b)[0])
        raise AssertionError(("candidate", where, k, a[k], b[k]))


def check_rows(markers, counts, refs, defined, sizes, where):
    """device rows against per-frame reference records; returns (records, poses compared, worst pose difference)"""
    n = n_pose = 0
    worst = 0.0
    for f, (ref, ok) in enumerate(zip(refs, defined)):
        assert counts[f] == len(ref), ("count", where, f, int(counts[f]), len(ref))
        for k, r in enumerate(ref):
            m = markers[f, k]
            assert (m["templateId"], m["markerId"], m["score"]) == (r.templateId, r.markerId, r.score), ("ids", where, f, k)
            assert np.array_equal(m["square"], np.array(r.square, np.float32)), ("square", where, f, k)
            w, h = sizes[r.templateId]
            assert m["aspectRatio"] == r.aspectRatio == w / h, ("aspectRatio", where, f, k, float(m["aspectRatio"]), w / h)
            n += 1
            if ok[k]:
                g = np.array(r.glMatrix)
                rel = np.abs(m["glMatrix"] - g).max() / max(1.0, np.abs(g).max())
                assert rel <= POSE_RTOL, ("pose", where, f, k, rel)
                worst = max(worst, rel)
                n_pose += 1
    return n, n_pose, worst


def check_records(det, markers, counts, runs, which, where):
    n, n_pose, worst = check_rows(markers, counts, [r.ref for r in runs], [r.defined for r in runs], NS.SIZES[which], where)
    n_cands = 0
    for f, r in enumerate(runs):
        check_candidates(det.debug_candidates(f), r.cands, (where, f))
        n_cands += len(r.cands)
    print("\n%s: %d frames, %d records (%d poses compared, %d excluded), %d candidates, worst pose difference %.2g" % (
        where, len(runs), n, n_pose, n - n_pose, n_cands, worst))
    return n, n_pose


@pytest.mark.parametrize("family", ["pinhole", "lens"])
def test_stateless_library_a(oa, family):
    runs = NS.runs("A", family)
    det = detector(oa, "A", runs[0].scene.cam)
    d = device_frames([r.scene for r in runs])
    markers, counts = det.detect_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, len(runs))
    n, n_pose = check_records(det, markers, counts, runs, "A", "library A, " + family)
    assert n == n_pose and n >= 16   # no record of a tilted frame is excluded


@pytest.mark.parametrize("family", ["pinhole", "lens"])
def test_extreme_shapes_library_b(oa, family):
    """every square of the frames through the 16 patch shapes of library B (64x1 ... 1x63): every bit the oracle's"""
    runs = NS.runs("B", family)
    det = detector(oa, "B", runs[0].scene.cam)
    d = device_frames([r.scene for r in runs])
    markers, counts = det.detect_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, len(runs))
    check_records(det, markers, counts, runs, "B", "library B, " + family)
    bits = [c.bit for r in runs for c in r.cands]
    assert len(bits) >= 16 * 16 * 3 and any(b < 0 for b in bits)


def test_frontal_frames(oa):
    runs = NS.runs("A", "frontal")
    det = detector(oa, "A", runs[0].scene.cam, batch=len(runs))
    d = device_frames([r.scene for r in runs])
    markers, counts = det.detect_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, len(runs))
    n, n_pose = check_records(det, markers, counts, runs, "A", "frontal")
    assert 1 <= n - n_pose and 2 * n_pose >= n


def test_tracked_steps_carry_the_ratio(oa):
    """two enqueue_tracked steps over the tilted pinhole frames, step 1's records step 2's prev"""
    import torch
    runs = NS.runs("A", "pinhole")
    S = len(runs)
    cam, tpls = runs[0].scene.cam, NS.library("A")[1]
    step2 = [H.oracle_registration(r.scene.frame, tpls, cam, prev=r.ref, max_cands=48 * len(tpls))[0] for r in runs]
    defined2 = [[NS.pose_is_defined(np.array(m.square, np.float32), m.aspectRatio, cam) for m in ref] for ref in step2]
    assert all(all(ok) for ok in defined2)
    det = detector(oa, "A", cam, batch=S)
    M = det.max_markers
    d_prev = torch.zeros((S, M, oa.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    d = device_frames([r.scene for r in runs])
    for step, (refs, ok) in enumerate((([r.ref for r in runs], [r.defined for r in runs]), (step2, defined2))):
        det.enqueue_tracked(d.data_ptr(), NS.WIDTH, NS.HEIGHT, S, d_prev.data_ptr(), d_cnt.data_ptr())
        m, c = det.collect()
        n, n_pose, worst = check_rows(m, c, refs, ok, NS.SIZES_A, ("tracked", step))
        print("\ntracked step %d: %d records, worst pose difference %.2g" % (step, n, worst))
        assert n == n_pose
        d_prev.copy_(torch.from_numpy(m.view(np.uint8).reshape(S, M, -1)).to("cuda:0"))
        d_cnt.copy_(torch.from_numpy(np.minimum(c, M).astype(np.int32)).to("cuda:0"))
    # step 2 reports carried records: more than step 1 found, each with its template's ratio (checked above)
    assert sum(len(r) for r in step2) > sum(len(r.ref) for r in runs)


def test_dense_context_gives_the_same_records(oa):
    """decode_kernel<true> and finalise_kernel<true>: the records of the plain context, byte for byte"""
    runs = NS.runs("A", "pinhole")[:4]
    d = device_frames([r.scene for r in runs])
    plain = detector(oa, "A", runs[0].scene.cam, batch=4)
    m0, c0 = plain.detect_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, 4)
    dense = detector(oa, "A", runs[0].scene.cam, batch=4, max_quads=1024, max_markers=512)
    m1, c1 = dense.detect_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, 4)
    check_records(dense, m1, c1, runs, "A", "dense")
    assert np.array_equal(c0, c1)
    for f in range(4):
        assert m0[f, :c0[f]].tobytes() == m1[f, :c1[f]].tobytes(), f


def test_corner_refinement_on(oa):
    """refinement (5, 30, 0.1) against the host chain of tests/refine_chain.py, which solves the pose of the refined square at
    the record's aspectRatio: squares bit-exact, poses where the reference defines them for the refined square"""
    import refine_chain as RC
    L = RC.build_emul()
    runs = NS.runs("A", "pinhole")
    cam = runs[0].scene.cam
    exp = [RC.refined_markers(L, r.ref, r.gray, cam, (5, 30, 0.1)) for r in runs]
    defined = [[NS.pose_is_defined(np.array(m.square, np.float32), m.aspectRatio, cam) for m in e] for e in exp]
    det = detector(oa, "A", cam)
    det.set_corner_refine(5, 30, 0.1)
    d = device_frames([r.scene for r in runs])
    markers, counts = det.detect_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, len(runs))
    n, n_pose, worst = check_rows(markers, counts, exp, defined, NS.SIZES_A, "refined")
    moved = sum(bytes(e.square) != bytes(r.square) for ex, run in zip(exp, runs) for e, r in zip(ex, run.ref))
    print("\nrefined: %d records (%d moved, %d poses compared), worst pose difference %.2g" % (n, moved, n_pose, worst))
    assert moved >= n // 2 and n_pose >= n // 2


def test_pipe_submit_collect_and_track(oa):
    """Pipe.submit/collect over the 16 tilted pinhole frames in chunks of 2 on 3 contexts, then two Pipe.track_device steps of
    6 streams: the records of the single context (the oracle's)"""
    import torch
    runs = NS.runs("A", "pinhole")
    cam, tpls = runs[0].scene.cam, NS.library("A")[1]
    pipe = oa.Pipe(NS.WIDTH, NS.HEIGHT, chunk_frames=2, n_contexts=3, gate_width=1)
    pipe.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    pipe.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    d = device_frames([r.scene for r in runs])
    fb = NS.WIDTH * NS.HEIGHT * 3
    n = 0
    for first in range(0, 8, 3):
        chunks = range(first, min(first + 3, 8))
        for s in chunks:
            assert pipe.submit(d.data_ptr() + 2 * s * fb, NS.WIDTH, NS.HEIGHT, 2, tag=s)
        for s in chunks:
            tag, m, c = pipe.collect(2)
            assert tag == s
            n += check_rows(m, c, [r.ref for r in runs[2 * s:2 * s + 2]], [r.defined for r in runs[2 * s:2 * s + 2]],
                            NS.SIZES_A, ("submit/collect", s))[0]
    assert n == sum(len(r.ref) for r in runs)
    S = 6
    prev = [None] * S
    for t in range(2):
        markers, counts = pipe.track_device(d.data_ptr(), NS.WIDTH, NS.HEIGHT, S, reset=(t == 0))
        refs = [H.oracle_registration(runs[s].scene.frame, tpls, cam, prev=prev[s], max_cands=48 * len(tpls))[0] for s in range(S)]
        ok = [[NS.pose_is_defined(np.array(m.square, np.float32), m.aspectRatio, cam) for m in ref] for ref in refs]
        assert all(all(o) for o in ok)
        check_rows(markers, counts, refs, ok, NS.SIZES_A, ("track", t))
        prev = refs
    assert sum(len(p) for p in prev) > sum(len(r.ref) for r in runs[:S])


def test_host_mirror_registration_with_templates_from_png(oa, tmp_path):
    """cvarArMultRegistration of libopencv-ar.so on two tilted frames, library A loaded from non-square PNG files"""
    import ctypes as C
    import os
    import subprocess
    host = C.CDLL(os.path.join(H.PKG, "lib", "libopencv-ar.so.1.0.0"))
    loaded = NS.templates_from_png(host, tmp_path)
    tpls = (H.Template * len(loaded))(*loaded)
    assert bytes(tpls) == bytes(NS.library("A")[1])
    exe = host_driver("registration_driver")
    for f, r in enumerate(NS.runs("A", "pinhole")[:2]):
        inp, out = tmp_path / ("in%d.bin" % f), tmp_path / ("out%d.bin" % f)
        inp.write_bytes(np.array([NS.WIDTH, NS.HEIGHT, len(tpls)], np.int32).tobytes() + bytes(tpls) + bytes(r.scene.cam) +
                        r.scene.frame.tobytes())
        p = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        raw = out.read_bytes()
        count, n_out = np.frombuffer(raw[:8], np.int32)
        markers = np.frombuffer(raw[8:], oa.MARKER_DTYPE).reshape(1, -1)
        assert n_out == count
        n, n_pose, _ = check_rows(markers, [count], [r.ref], [r.defined], NS.SIZES_A, ("cvarArMultRegistration", f))
        assert n >= 1 and n == n_pose

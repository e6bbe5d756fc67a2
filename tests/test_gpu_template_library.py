"""GPU tests of template libraries beyond 16 templates (up to OCVAR_MAX_TEMPLATES = 4096, at most 16 code sizes): synthetic
scenes whose markers are drawn from random code grids, against the oracle (which takes any number of templates).  Every
frame's markers (ids, score, corners bit-exact, pose within 1e-4) and every pre-elimination candidate must match, through
Detector.detect_device, Pipe.submit/collect, Pipe.track_device and cvarArMultRegistration of libopencv-ar.so."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import helpers as H
from frame_kit import E_ARG, oa  # noqa: F401
from hostbuild import host_driver

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4


_libraries = {}


def library(kind, n):
    """names of n registered random templates (cached): kind 'r8' 8x8 codes, 'mixed' 2x2 .. 8x8, 'dupsym' 8x8 codes with
    repeated templates and rotationally symmetric ones"""
    key = (kind, n)
    if key in _libraries:
        return _libraries[key]
    rng = np.random.default_rng([n, len(kind)])
    names, grids = [], []
    for i in range(n):
        name = f"{kind}-{n}-{i}"
        if kind == "r8":
            g = rng.integers(0, 2, (8, 8))
        elif kind == "mixed":
            w = 2 + i % 7
            g = rng.integers(0, 2, (w, w))
        else:
            r = i % 5
            if r == 1 and i > 5:
                g = grids[int(rng.integers(0, i))]          # a repeat of an earlier template
            elif r == 3:
                q = rng.integers(0, 2, (4, 4))
                g = np.zeros((8, 8), np.int64)
                g[:4, :4] = q
                for _ in range(3):                         # 4-fold symmetric: all four codes equal
                    g = np.maximum(g, np.rot90(g))
            elif r == 4:
                h = rng.integers(0, 2, (4, 8))
                g = np.concatenate([h, np.rot90(h, 2)])   # 2-fold symmetric: code[0] == code[2]
            else:
                g = rng.integers(0, 2, (8, 8))
        H.register_template(name, g)
        names.append(name)
        grids.append(g)
    tpls = H.oracle_templates(names)
    _libraries[key] = (names, tpls)
    return names, tpls


def scenes(names, plants, width=640, height=480, rot_mode=0):
    """one frame per plant list (2 x 2 markers of the listed templates, in order)"""
    cfg = H.synth_config(2, width=width, height=height, rot_mode=rot_mode)
    frames = np.stack([H.synth_frame(cfg, 4 * f, [names[t] for t in p])[0] for f, p in enumerate(plants)])
    return cfg, frames


def oracle(frame, tpls, prev=None):
    w, h = frame.shape[1], frame.shape[0]
    m, c, _ = H.oracle_registration(frame, tpls, H.oracle_camera(w, h), prev=prev, max_cands=48 * len(tpls))
    return m, c


def check_markers(row, count, ref, where):
    assert count == len(ref), ("count", where, int(count), len(ref))
    for k, r in enumerate(ref):
        m = row[k]
        assert (m["templateId"], m["markerId"], m["score"]) == (r.templateId, r.markerId, r.score), ("marker", where, k)
        assert np.array_equal(m["square"], np.array(r.square, np.float32)), ("corners", where, k)
        assert m["aspectRatio"] == r.aspectRatio, ("aspectRatio", where, k)
        g = np.array(r.glMatrix)
        assert np.abs(m["glMatrix"] - g).max() <= POSE_RTOL * max(1.0, np.abs(g).max()), ("pose", where, k)


CAND = np.dtype(H.Candidate)
CAND_FIELDS = ["markerId", "templateId", "orient", "bit", "square", "patPoint"]


def check_candidates(cands, ref, where):
    assert len(cands) == len(ref), ("candidate count", where, len(cands), len(ref))
    a = np.frombuffer(b"".join(bytes(c) for c in cands), CAND)[CAND_FIELDS]
    b = np.frombuffer(b"".join(bytes(c) for c in ref), CAND)[CAND_FIELDS]
    if not np.array_equal(a, b):
        k = int(np.flatnonzero(a != b)[0])
        raise AssertionError(("candidate", where, k, a[k], b[k]))


def detector(oa, cfg, tpls, batch):
    det = oa.Detector(cfg.width, cfg.height, max_batch=batch)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(cfg.width, cfg.height))))
    return det


def detect_and_check(oa, names, tpls, plants, **kw):
    import torch
    cfg, frames = scenes(names, plants, **kw)
    det = detector(oa, cfg, tpls, len(frames))
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    markers, counts = det.detect_device(d.data_ptr(), cfg.width, cfg.height, len(frames))
    n_markers = n_cands = 0
    for f in range(len(frames)):
        ref_m, ref_c = oracle(frames[f], tpls)
        check_markers(markers[f], counts[f], ref_m, ("frame", f))
        check_candidates(det.debug_candidates(f), ref_c, ("frame", f))
        n_markers += len(ref_m)
        n_cands += len(ref_c)
    return n_markers, n_cands


def test_17_templates_one_past_the_old_cap(oa):
    names, tpls = library("r8", 14)
    names = H.TEMPLATE_ORDER + names
    tpls = H.oracle_templates(names)
    assert len(tpls) == 17
    plants = [[0, 1, 2, 16], [16, 3, 16, 0], [5, 9, 0, 12], [1, 1, 7, 15]]
    n_markers, n_cands = detect_and_check(oa, names, tpls, plants)
    assert n_markers >= 8 and n_cands >= 12 * 17


@pytest.mark.parametrize("K", [1024, 4096])
def test_large_libraries(oa, K):
    names, tpls = library("r8", K)
    # template 0 on a later square (it removes a score-0 survivor), the last template, repeats within a frame
    plants = [[K - 1, 7, 0, K // 2], [3, 3, K - 1, 0], [0, 0, 1, 2]]
    n_markers, _ = detect_and_check(oa, names, tpls, plants, rot_mode=0)
    assert n_markers >= 6


def test_mixed_size_library(oa):
    names, tpls = library("mixed", 70)   # 2x2 .. 8x8, ten of each
    assert len({(t.width, t.height) for t in tpls}) == 7
    plants = [[0, 1, 2, 3], [4, 5, 6, 7], [69, 62, 14, 0], [8, 15, 22, 29]]
    n_markers, _ = detect_and_check(oa, names, tpls, plants)
    assert n_markers >= 10


def test_duplicate_and_symmetric_codes(oa):
    names, tpls = library("dupsym", 60)
    codes = [tuple(t.code) for t in tpls]
    assert len(set(codes)) < len(codes)                       # repeated templates
    assert any(len(set(c)) == 1 for c in codes) and any(c[0] == c[2] and c[0] != c[1] for c in codes)
    dup = next(i for i in range(len(codes)) if codes.index(codes[i]) != i)
    plants = [[3, 8, 4, 9], [dup, codes.index(codes[dup]), 13, 0], [13, 14, 18, 19], [dup, 3, 3, 0]]
    n_markers, _ = detect_and_check(oa, names, tpls, plants)
    assert n_markers >= 6


def test_pipe_submit_collect_and_track_with_1024_templates(oa):
    import torch
    K = 1024
    names, tpls = library("r8", K)
    plants = [[0, 1, 2, 3], [K - 1, 0, 10, 10], [500, 501, 0, 2], [9, 8, 7, 6], [3, 3, 3, 3], [1, 600, 0, K - 2]]
    cfg, frames = scenes(names, plants)
    cam = oa.Camera.from_buffer_copy(bytes(H.oracle_camera(cfg.width, cfg.height)))
    pipe = oa.Pipe(cfg.width, cfg.height, chunk_frames=2, n_contexts=3, gate_width=1)
    pipe.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    pipe.set_camera(cam)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    fb = cfg.width * cfg.height * 3
    for s in range(3):
        assert pipe.submit(d.data_ptr() + 2 * s * fb, cfg.width, cfg.height, 2, tag=s)
    refs = [oracle(frames[f], tpls)[0] for f in range(len(frames))]
    for s in range(3):
        tag, m, c = pipe.collect(2)
        assert tag == s
        for k in range(2):
            check_markers(m[k], c[k], refs[2 * s + k], ("submit/collect", 2 * s + k))
    # three time steps of 3 streams: the streams' markers of the previous step are tracked on the device
    seq = [[0, 0, 1], [2, 2, 2], [4, 5, 5]]
    prev = [None] * 3
    for t in range(3):
        step = np.ascontiguousarray(np.stack([frames[seq[s][t]] for s in range(3)]))
        ds = torch.from_numpy(step).cuda()
        torch.cuda.synchronize()
        markers, counts = pipe.track_device(ds.data_ptr(), cfg.width, cfg.height, 3, reset=(t == 0))
        for s in range(3):
            ref, _ = oracle(step[s], tpls, prev=prev[s])
            check_markers(markers[s], counts[s], ref, ("track", t, s))
            prev[s] = ref
    assert max(len(p) for p in prev) >= 2


def test_host_mirror_registration_with_100_templates(oa, tmp_path):
    names, tpls = library("r8", 100)
    cfg, frames = scenes(names, [[99, 0, 50, 0]])
    exe = host_driver("registration_driver")
    cam = H.oracle_camera(cfg.width, cfg.height)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array([cfg.width, cfg.height, len(tpls)], np.int32).tobytes() + bytes(tpls) + bytes(cam) + frames[0].tobytes())
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    count, n_out = np.frombuffer(raw[:8], np.int32)
    markers = np.frombuffer(raw[8:], oa.MARKER_DTYPE)
    ref, _ = oracle(frames[0], tpls)
    assert n_out == count
    check_markers(markers, count, ref, "cvarArMultRegistration")
    assert count >= 2


def test_set_templates_limits(oa):
    names, tpls = library("r8", 1024)
    lib = oa.hip_lib()
    det = oa.Detector(64, 64, max_batch=1)
    arr = (oa.Template * 4097)(*([oa.Template.from_buffer_copy(bytes(t)) for t in tpls] * 5)[:4097])
    assert lib.ocvar_hip_set_templates(det._ctx, arr, 4097) == E_ARG
    assert lib.ocvar_hip_set_templates(det._ctx, arr, 4096) == 0
    # 17 distinct code sizes; 16 are accepted
    sizes = [(w, h) for w in range(1, 9) for h in (1, 2)] + [(3, 3)]
    arr17 = (oa.Template * 17)()
    for i, (w, h) in enumerate(sizes):
        arr17[i].width, arr17[i].height, arr17[i].scale = w, h, 0.01
        arr17[i].code[0] = i
    assert lib.ocvar_hip_set_templates(det._ctx, arr17, 17) == E_ARG
    assert "sizes" in lib.ocvar_hip_last_error(det._ctx).decode()
    assert lib.ocvar_hip_set_templates(det._ctx, arr17, 16) == 0
    pipe = oa.Pipe(64, 64, chunk_frames=1, n_contexts=2, gate_width=1)
    with pytest.raises(oa.OcvarError):
        pipe.set_templates(list(arr17))
    pipe.set_templates(list(arr)[:4096])

"""GPU tests of every way a batch is cut into work units (scenes and case tables: tests/work_cut_scenes.py, whose classes
tests/test_work_cuts_cpu.py proves present): the crop binarise kernel's planes, read back bit for bit; the frame kernel at its
chunk seams; and results that do not depend on the batch plan, the tuning knobs, the streams or the gate.  Everything is compared
bit for bit with the oracle (poses: POSE_RTOL of test_gpu_parity.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import work_cut_scenes as S
from frame_kit import E_ARG, oa  # noqa: F401
from geometry_scenes import pinhole_camera
from test_batch_plan_cpu import lib, plan   # noqa: F401  (lib: the fixture that builds tests/emul/plan_emul.cpp)
from test_gpu_input_formats import as_format
from test_gpu_parity import OracleFrame, cand_array, check_candidates, check_markers, check_planes, make_detector

pytestmark = pytest.mark.gpu


def size(w, h):
    return SimpleNamespace(width=w, height=h)


# ---- B: the crop pass's planes ------------------------------------------------------------------------------------------------
_crop_refs = {}


def crop_refs(name, tpls, cam):
    if name not in _crop_refs:
        _crop_refs[name] = [OracleFrame(f, tpls, cam) for f in S.crop_scene(name)[2]]
    return _crop_refs[name]


def check_crops(det, refs, W, Hh, want, where):
    """the crop ROIs of det's last batch against crop_rect on the frame pass's quads, and both planes of every crop against the
    oracle's binarise of the same rectangle of the oracle's grey frame"""
    rois = det.debug_crops()
    per_frame = [[] for _ in refs]
    for r in rois:
        per_frame[int(r["frame"])].append(tuple(int(r[k]) for k in ("owner", "x0", "y0", "w", "h")))
    for f, ref in enumerate(refs):
        quads = det.debug_frame_quads(f)
        assert np.array_equal(quads, ref.quads), ("frame quads", where, f)
        assert sorted(per_frame[f]) == sorted(S.crop_rois(quads, W, Hh)), ("crop ROIs", where, f)
    got = S.crop_classes(per_frame, W, Hh)
    assert want <= got, ("classes the read-back crops reach", where, sorted(want - got))
    assert [int(r["index"]) for r in rois] == list(range(len(rois)))
    for r in rois:
        f, x0, y0, w, h = (int(r[k]) for k in ("frame", "x0", "y0", "w", "h"))
        binary = H.oracle_binarise(np.ascontiguousarray(refs[f].grey[y0:y0 + h, x0:x0 + w]))
        masks = H.neighbour_masks(binary)
        binary[0, :] = binary[-1, :] = 0   # (the plane is stored with cvFindContours' zeroed frame)
        binary[:, 0] = binary[:, -1] = 0
        got_b, got_m = det.debug_crop_binary(r), det.debug_crop_masks(r)
        assert got_b.shape == binary.shape and np.array_equal(got_b, binary), ("crop binary image", where, f, (x0, y0, w, h), np.argwhere(got_b != binary)[:4].tolist())
        assert np.array_equal(got_m, masks), ("crop mask plane", where, f, (x0, y0, w, h), np.argwhere(got_m != masks)[:4].tolist())
    return len(rois)


@pytest.mark.parametrize("name", sorted(S.CROP_SCENES))
def test_crop_planes_against_the_oracle(oa, name):
    W, Hh, frames, want = S.crop_scene(name)
    n = len(frames)
    det, tpls, cam = make_detector(oa, size(W, Hh), None, n)
    refs = crop_refs(name, tpls, cam)
    markers, counts = det.detect_host(frames.copy())
    assert check_crops(det, refs, W, Hh, want, name) >= n // 2
    for f in range(n):
        check_planes(det, f, refs[f], where=name)
        check_candidates(det, f, refs[f], where=name)
        check_markers(f, refs[f], markers, counts, where=name)
    det.close()


def test_crop_planes_of_a_full_pool_on_a_dense_context(oa):
    """the frame of a hundred markers among eight others, on a context made by ocvar_hip_create_dense"""
    W, Hh, frames, want = S.crop_scene("pool")
    n = len(frames)
    tpls, cam = H.oracle_templates(), H.oracle_camera(W, Hh)
    det = oa.Detector(W, Hh, max_batch=n, max_quads=300, max_markers=128)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    refs = crop_refs("pool", tpls, cam)
    markers, counts = det.detect_host(frames.copy())
    assert check_crops(det, refs, W, Hh, want, "pool, dense") >= 100
    for f in range(n):
        check_candidates(det, f, refs[f], where="pool, dense")
        check_markers(f, refs[f], markers, counts, where="pool, dense")
    det.close()


def test_crop_read_back_refuses_what_it_cannot_give(oa):
    import torch
    W, Hh, frames, _ = S.crop_scene("panels")
    det, tpls, cam = make_detector(oa, size(W, Hh), None, 2)
    with pytest.raises(oa.OcvarError):     # no batch has been collected
        det.debug_crops()
    d = torch.from_numpy(frames[:2]).cuda()
    det.enqueue_device(d.data_ptr(), W, Hh, 2)
    with pytest.raises(oa.OcvarError):     # in flight
        det.debug_crops()
    det.collect()
    rois = det.debug_crops()
    assert len(rois) >= 2
    for bad in (-1, len(rois), 1 << 30):
        out = np.zeros((Hh, W), np.uint8)
        assert det._lib.ocvar_hip_debug_crop_plane(det._ctx, bad, 0, out.ctypes.data) == E_ARG
    assert det._lib.ocvar_hip_debug_crop_plane(det._ctx, 0, 0, None) == E_ARG
    # the first max_rois records, the full count
    one = np.zeros(1, oa.CROP_ROI_DTYPE)
    cnt = np.zeros(1, np.int32)
    assert det._lib.ocvar_hip_debug_crop_rois(det._ctx, one.ctypes.data, 1, cnt.ctypes.data) == 0
    assert cnt[0] == len(rois) and one[0] == rois[0]
    big = next(r for r in rois if r["w"] > 480).copy()          # (frame 0's large marker: no later frame has such a crop)
    det.detect_host(frames[2:4].copy())
    with pytest.raises(ValueError):        # a record of an earlier batch
        det.debug_crop_binary(big)
    det.find_squares(np.ascontiguousarray(frames[0][..., 0]))   # a batch without a crop pass
    with pytest.raises(oa.OcvarError):
        det.debug_crops()
    det.close()


# ---- C: the frame kernel at its chunk seams -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CHUNK_CASES, ids=["%dx%d-%s" % (c[0], c[1], "default" if c[2] is None else "min_units%d" % c[2]) for c in S.CHUNK_CASES])
def test_frame_kernel_at_its_chunk_seams(oa, lib, case):   # noqa: F811
    width, height, min_units, formats, want = case
    p = plan(lib, width, height, 1, max_batch=9) if min_units is None else plan(lib, width, height, 1, max_batch=9, min_units=min_units)
    assert want <= S.chunk_classes(width, height, min_units, plan(lib, width, height, 1, max_batch=9), p)
    base = S.chunk_frames(width, height, S.seam_rows(p), 7 * width + height)
    # (a pinhole camera: cvarCameraScale would stretch the 4:3 default to these frames' 1:20, where the planar pose fit has no
    # well-defined minimum and two solvers end in different places -- DESIGN.md section 5)
    tpls, cam = H.oracle_templates(), pinhole_camera(width, height)
    refs = {}
    for fmt in formats:
        pairs = [as_format(b, fmt, 31 + i) for i, b in enumerate(base)]
        key = "gray" if fmt == "gray" else "colour"   # (the colour formats hold the same colours)
        if key not in refs:
            refs[key] = [OracleFrame(pr[1], tpls, cam) for pr in pairs]
        det, _, _ = make_detector(oa, size(width, height), None, 9)
        det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
        det.set_input_format(fmt)
        for n, order in ((1, [0]), (1, [1]), (9, [0, 1, 1, 0, 1, 0, 0, 1, 1])):
            if min_units is not None:
                det.set_tuning(min_units=min_units * n)   # (the plan counts units over the batch: the same cut at 9 frames)
            markers, counts = det.detect_host(np.stack([pairs[u][0] for u in order]))
            for f, u in enumerate(order):
                where = (width, height, min_units, fmt, n, f, "noise" if u == 0 else "seam markers")
                check_planes(det, f, refs[key][u], where=where)
                check_candidates(det, f, refs[key][u], where=where)
                check_markers(f, refs[key][u], markers, counts, where=where)
        det.close()


# ---- D: results do not depend on the plan ---------------------------------------------------------------------------------------
PW, PH, PU, PMAX = 320, 240, 8, 129
PFB = PW * PH * 3


@pytest.fixture(scope="module")
def ps(oa):
    """the plan scene on the device, tiled to the largest batch, its poison, the oracle's results per distinct frame, and the
    records of the first run of each distinct frame, which every later run must repeat byte for byte"""
    import torch
    frames, poison = S.plan_scene()
    tpls, cam = H.oracle_templates(), H.oracle_camera(PW, PH)
    idx = torch.arange(PMAX + PU) % PU
    return SimpleNamespace(oa=oa, tpls=tpls, cam=cam, refs=[OracleFrame(f, tpls, cam, planes=False) for f in frames],
                           d=torch.from_numpy(frames)[idx].contiguous().cuda(), d_poison=torch.from_numpy(poison)[idx].contiguous().cuda(),
                           first={})


def plan_detector(ps, max_batch, gate=None):
    det, _, _ = make_detector(ps.oa, size(PW, PH), None, max_batch)
    if gate is not None:
        det.set_gate(gate)
    return det


def verify(ps, det, markers, counts, n, u0, where):
    """batch position f holds distinct frame (u0 + f) % 8: the oracle's candidates and markers, and the same bytes as ever"""
    for f in range(n):
        u = (u0 + f) % PU
        if f < PU:
            check_candidates(det, f, ps.refs[u], where=where)
            check_markers(f, ps.refs[u], markers, counts, where=where)
        got = (int(counts[f]), markers[f, :counts[f]].tobytes(), cand_array(det.debug_candidates(f)).tobytes())
        assert got == ps.first.setdefault(u, got), ("records differ from the first run's", where, f, u)


def poison(ps, det, n, stream=None):
    det.enqueue_device(ps.d_poison.data_ptr(), PW, PH, n, stream=stream)
    det.collect()


def run(ps, det, n, u0=0, where="", stream=None, between=None):
    """a batch of other frames through the context, then frames u0 .. u0 + n - 1 of the tiled scene"""
    poison(ps, det, n, stream)
    det.enqueue_device(ps.d.data_ptr() + u0 * PFB, PW, PH, n, stream=stream)
    if between is not None:
        between(det)
    markers, counts = det.collect()
    verify(ps, det, markers, counts, n, u0, where)
    return markers, counts


def stage_times_are_sane(det, where):
    ms = det.stage_ms()
    assert len(ms) == 12 and np.isfinite(ms).all() and (ms >= 0).all(), (where, ms.tolist())


@pytest.mark.parametrize("n", [1, 7, 8, 9, 16, 17, 127, 128, 129])
def test_results_across_batch_sizes(ps, n):
    for max_batch in (n, 256):
        det = plan_detector(ps, max_batch)
        run(ps, det, n, where=("batch", n, max_batch))
        det.close()


KNOBS = [("mid_steps", (32, 97, 128, 1536, 100000)), ("mid_blocks", (1, 32)), ("long_blocks", (1,)), ("short_blocks", (1, 65535)),
         ("crop_phases", (1, 2)), ("min_units", (1, 2))]   # (mid_blocks 32: the most a context of 9 frames has)


@pytest.mark.parametrize("knob,values", KNOBS, ids=[k for k, _ in KNOBS])
def test_results_across_tuning_knobs(ps, knob, values):
    det = plan_detector(ps, 9)
    for v in values:
        det.set_tuning(**{knob: v})
        for u in range(PU):
            run(ps, det, 1, u0=u, where=(knob, v, 1, u))
        run(ps, det, 9, where=(knob, v, 9))
    det.set_tuning(**{knob: 0})
    run(ps, det, 9, where=(knob, "default"))
    det.close()


HP_MASKS = [1 << k for k in range(9)] + [0x1ff, 0x155, 0x0aa]


@pytest.mark.parametrize("mode", ["own_stream", "callers_stream", "two_contexts_on_a_gate", "copies_and_drawing_in_between"])
def test_results_across_high_priority_masks(ps, mode):
    import torch
    from opencv_ar_amd import sharding as Sh
    oa, n = ps.oa, 9
    gate = oa.Gate(2) if mode == "two_contexts_on_a_gate" else None
    dets = [plan_detector(ps, n, gate) for _ in range(2 if gate is not None else 1)]
    stream = torch.cuda.Stream() if mode == "callers_stream" else None
    sptr = stream.cuda_stream if stream is not None else None
    block = torch.zeros(Sh.block_bytes(n), dtype=torch.uint8, device="cuda")
    canvas = ps.d[:n].clone()
    torch.cuda.synchronize()

    def between(det):
        det.results_to_device(block.data_ptr(), block.data_ptr() + n * Sh.MAX_MARKERS * Sh.MARKER_BYTES)
        det.annotate(canvas.data_ptr(), PW, PH)

    def one(where):
        if gate is not None:   # both contexts in flight at once, on the gate's lanes
            for k, det in enumerate(dets):
                poison(ps, det, n)
            for k, det in enumerate(dets):
                det.enqueue_device(ps.d.data_ptr() + k * PFB, PW, PH, n)
            for k, det in enumerate(dets):
                markers, counts = det.collect()
                verify(ps, det, markers, counts, n, k, where)
                stage_times_are_sane(det, where)
            return
        markers, counts = run(ps, dets[0], n, where=where, stream=sptr, between=between if mode == "copies_and_drawing_in_between" else None)
        stage_times_are_sane(dets[0], where)
        if mode == "copies_and_drawing_in_between":
            torch.cuda.synchronize()
            res = Sh.unpack([block], n, oa.MARKER_DTYPE)
            for f in range(n):
                assert res[f][0] == counts[f] and res[f][1].tobytes() == markers[f, :counts[f]].tobytes(), (where, f)

    for mask in HP_MASKS:
        for det in dets:
            det.set_tuning(hp_mask=mask)
        for rep in range(2):
            one((mode, hex(mask), rep))
    for det in dets:
        det.set_tuning(hp_mask=0)
    one((mode, "mask 0 again"))
    torch.cuda.synchronize()
    for det in dets:
        det.close()
    del dets, gate


@pytest.mark.parametrize("width", [1, 2])
def test_results_across_gate_modes(ps, width):
    oa, n = ps.oa, 9
    gate = oa.Gate(width)
    dets = [plan_detector(ps, n, gate) for _ in range(3)]
    for modes in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 1, 2), (2, 0, 1), (1, 2, 2)):
        for det, m in zip(dets, modes):
            det.set_tuning(gate_mode=m)
        for det in dets:
            det.enqueue_device(ps.d_poison.data_ptr(), PW, PH, n)
        for det in dets:
            det.collect()
        for k, det in enumerate(dets):
            det.enqueue_device(ps.d.data_ptr() + 3 * k * PFB, PW, PH, n)
        for k in (1, 0, 2):
            markers, counts = dets[k].collect()
            verify(ps, dets[k], markers, counts, n, 3 * k, ("gate", width, modes, k))
            stage_times_are_sane(dets[k], ("gate", width, modes, k))
    for det in dets:
        det.close()
    del dets, gate

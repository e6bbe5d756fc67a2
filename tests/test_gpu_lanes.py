"""The gate as the scheduler of its contexts' batches (include/ocvar_hip.h: lanes) on the GPU: five contexts, gate 2, ragged
launches as in test_gpu_load.py, with 1, 2 and 4 lanes -- every frame's markers and count equal to the same frame on one
ungated context, whatever lane carried it and in whatever order the contexts are collected."""
import os

import numpy as np
import pytest

import helpers as H

NS, GATE, LAUNCH, U = 5, 2, 40, 48
NAMES = ["2x2-01"]


@pytest.fixture(scope="module")
def scene():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    import opencv_ar_amd as oa
    cfg = H.synth_config(2)
    tpls = oa.load_templates([os.path.join(oa.TEMPLATE_DIR, x + ".png") for x in NAMES])
    cam = oa.default_camera(cfg.width, cfg.height)
    base = np.stack([H.synth_frame(cfg, 11 * f, NAMES)[0] for f in range(U)])
    d_base = torch.from_numpy(base).cuda()
    n_dev = 2 * LAUNCH + 7 * NS
    d = d_base[torch.arange(n_dev, device="cuda") % U].contiguous()
    torch.cuda.synchronize()
    det = oa.Detector(cfg.width, cfg.height, max_batch=U)   # the yardstick: one context, no gate, one batch
    det.set_templates(tpls)
    det.set_camera(cam)
    ref_m, ref_c = det.detect_device(d_base.data_ptr(), cfg.width, cfg.height, U, max_per_frame=8)
    det.close()
    assert ref_c.min() >= 1
    return {"oa": oa, "cfg": cfg, "tpls": tpls, "cam": cam, "d": d, "d_base": d_base, "ref": (ref_m, ref_c),
            "fb": cfg.width * cfg.height * 3}


def same_as_ref(sc, got, j0, where):
    """frames j0 .. of the tiled array against the ungated context's results of the distinct frames they repeat"""
    m, c = got
    ref_m, ref_c = sc["ref"]
    for p in range(len(c)):
        u = (j0 + p) % U
        assert c[p] == ref_c[u], f"{where} position {p}: count {c[p]}, ungated {ref_c[u]}"
        assert m[p].tobytes() == ref_m[u].tobytes(), f"{where} position {p}: marker records differ from the ungated context's"


def make_dets(sc, gate, n=NS, max_batch=LAUNCH):
    dets = []
    for _ in range(n):
        det = sc["oa"].Detector(sc["cfg"].width, sc["cfg"].height, max_batch=max_batch)
        det.set_templates(sc["tpls"])
        det.set_camera(sc["cam"])
        det.set_gate(gate)
        det.set_result_limit(8)
        dets.append(det)
    return dets


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_ragged_launches_on_lanes_equal_one_ungated_context(scene, lanes):
    import torch
    sc, oa, cfg = scene, scene["oa"], scene["cfg"]
    w, h = cfg.width, cfg.height
    gate = oa.Gate(GATE, lanes=lanes)
    assert gate.lanes == lanes
    dets = make_dets(sc, gate)
    ref_event = torch.cuda.Event(enable_timing=True)
    ref_event.record()
    ref_event.synchronize()
    first = [max(1, ((i + 1) * LAUNCH) // NS) for i in range(NS)]
    shift = 7

    def ptr(j):
        return sc["d"].data_ptr() + j * sc["fb"]

    def stamps_increase(det, where):
        st = det.stage_stamps(ref_event.cuda_event)
        assert len(st) == 13 and st[0] >= 0 and (np.diff(st) >= 0).all(), f"{where}: stage stamps {st.tolist()}"
        ms = det.stage_ms()
        assert (ms >= 0).all() and abs(ms[11] - (st[12] - st[0])) <= 0.05 + 1e-3 * ms[11], f"{where}: {ms.tolist()} against {st.tolist()}"

    for i in range(NS):
        dets[i].enqueue_device(ptr(shift * i), w, h, first[i])
    # bench.py's order: collect the oldest, re-enqueue it at once behind the others
    for i in range(NS):
        same_as_ref(sc, dets[i].collect(8), shift * i, f"lanes {lanes} context {i} launch 0")
        stamps_increase(dets[i], f"lanes {lanes} context {i} launch 0")
        dets[i].enqueue_device(ptr(shift * i + first[i]), w, h, LAUNCH)
    # another order than the one they were enqueued in, the re-enqueued ones landing wherever there is least work
    for rnd, order in enumerate(([3, 0, 4, 1, 2], [4, 3, 2, 1, 0])):
        for i in order:
            same_as_ref(sc, dets[i].collect(8), shift * i + first[i], f"lanes {lanes} context {i} round {rnd}")
            stamps_increase(dets[i], f"lanes {lanes} context {i} round {rnd}")
            if rnd == 0 or i % 2:
                dets[i].enqueue_device(ptr(shift * i + first[i]), w, h, LAUNCH)
        if rnd == 1:
            for i in order:
                if i % 2:
                    same_as_ref(sc, dets[i].collect(8), shift * i + first[i], f"lanes {lanes} context {i} last")

    # frames written by a torch kernel on the context's stream right before the enqueue, nothing in between: those are the
    # frames detected.  (The stream is first kept busy, so that a batch which did not wait for it would read the zeros.)
    bufs = [torch.zeros((LAUNCH, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(NS)]
    a = torch.randn((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    for i in range(NS):
        ext = torch.cuda.ExternalStream(dets[i].stream_ptr())
        j0 = 3 * i
        with torch.cuda.stream(ext):
            b = a
            for _ in range(20):
                b = (b @ a) * 1e-3
            torch.add(sc["d"][j0:j0 + LAUNCH], 0, out=bufs[i])
        dets[i].enqueue_device(bufs[i].data_ptr(), w, h, LAUNCH)
    for i in (2, 0, 1, 4, 3):
        same_as_ref(sc, dets[i].collect(8), 3 * i, f"lanes {lanes} context {i} frames written on its stream")
    torch.cuda.synchronize()

    # a context goes on without the gate; the gate goes after its contexts
    dets[0].set_gate(None)
    same_as_ref(sc, dets[0].detect_device(ptr(5), w, h, LAUNCH, max_per_frame=8), 5, f"lanes {lanes} context 0 without its gate")
    dets[1].enqueue_device(ptr(9), w, h, LAUNCH)
    same_as_ref(sc, dets[1].collect(8), 9, f"lanes {lanes} context 1 beside a context that left the gate")
    for det in dets:
        det.close()
    del dets, det, gate


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_collect_covers_the_results_copy_on_the_contexts_stream(scene, lanes):
    """bench.py's multi-rank step: results_to_device on the context's own stream (or with no stream: on the lane), collect, and
    the gather reads the block from ANOTHER stream without waiting for anything -- the launches that filled it are complete.
    The context's stream is kept busy in front of the copy, so a collect that returned on the batch's kernels alone would
    leave the zeros in the block.  Every frame's count and records in the block equal collect's."""
    import torch
    sc, oa, cfg = scene, scene["oa"], scene["cfg"]
    w, h = cfg.width, cfg.height
    K = 8
    gate = oa.Gate(GATE, lanes=lanes)
    dets = make_dets(sc, gate)
    reader = torch.cuda.Stream()
    a = torch.randn((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    for rnd, own_stream in enumerate((True, False, True)):
        blk_m = [torch.zeros(LAUNCH * K * oa.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(NS)]
        blk_c = [torch.zeros(LAUNCH, dtype=torch.int32, device="cuda") for _ in range(NS)]
        torch.cuda.synchronize()
        for i in range(NS):
            dets[i].enqueue_device(sc["d"].data_ptr() + (4 * i + rnd) * sc["fb"], w, h, LAUNCH)
            ext = torch.cuda.ExternalStream(dets[i].stream_ptr())
            if own_stream:
                with torch.cuda.stream(ext):
                    b = a
                    for _ in range(20):
                        b = (b @ a) * 1e-3
            dets[i].results_to_device(blk_m[i].data_ptr(), blk_c[i].data_ptr(), ext.cuda_stream if own_stream else None, per_frame=K)
        for i in (1, 3, 0, 4, 2):
            m, c = dets[i].collect(K)
            with torch.cuda.stream(reader):   # (no wait for the context's stream, the lane or the device)
                got_m, got_c = blk_m[i].clone(), blk_c[i].clone()
            reader.synchronize()
            where = f"lanes {lanes} round {rnd} context {i}"
            same_as_ref(sc, (m, c), 4 * i + rnd, where)
            assert got_c.cpu().numpy().tobytes() == c.tobytes(), f"{where}: counts in the block differ from collect's"
            recs = got_m.cpu().numpy().view(oa.MARKER_DTYPE).reshape(LAUNCH, K)
            for p in range(LAUNCH):
                k = min(int(c[p]), K)
                assert recs[p, :k].tobytes() == m[p, :k].tobytes(), f"{where} position {p}: records in the block differ from collect's"
        torch.cuda.synchronize()
    for det in dets:
        det.close()
    del dets, det, gate


@pytest.mark.gpu
def test_default_lane_count_is_the_process_queue_count(scene):
    """the library reads GPU_MAX_HW_QUEUES (absent: the runtime's four) and opens that many lanes, eight at the most"""
    text = os.environ.get("GPU_MAX_HW_QUEUES", "")
    want = min(8, int(text)) if text.isdigit() and int(text) > 0 else 4
    gate = scene["oa"].Gate(GATE)
    assert gate.lanes == want

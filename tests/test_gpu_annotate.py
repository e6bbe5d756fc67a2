"""Annotation on the device (ocvar_hip_annotate / ocvar_hip_annotate_records) byte for byte against the host build of
annotate_core.h (tests/annotate_chain.py): whole buffers are compared, the guard bytes in the row padding, between the frames and
around the buffer included."""
import ctypes as C

import numpy as np
import pytest

import annotate_chain as AC
import frame_kit as FK
import helpers as H
import overlay_chain as OC
import persp_synth as PS
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return AC.build_emul()


@pytest.fixture(scope="module")
def LO():
    return OC.build_emul()


@pytest.fixture(scope="module")
def det320(oa):
    """a dense context of 130 markers per frame: record strides on both sides of the 64-slot ballot"""
    det = oa.Detector(320, 240, max_batch=4, max_markers=130)
    assert det.max_markers == 130
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam_of(320, 240, True))))
    return det


def cam_of(W, Hh, lens):
    return PS.camera(W, Hh, lens=lens)


def layout(n, W, Hh, fmt, aligned, seed=0):
    """guarded frames: aligned -- address and both strides multiples of 4; else the address is odd and so is the row stride"""
    bpp = FK.BPP[FK.FORMATS[fmt]]
    if aligned:
        p = FK.Frames(n, W, Hh, fmt, row_pad=4 + (-W * bpp) % 4, frame_gap=8, lead=FK.LEAD, seed=seed)
        assert p.row_stride % 4 == 0 and p.frame_stride % 4 == 0 and p.offset(0) % 4 == 0
    else:
        p = FK.Frames(n, W, Hh, fmt, row_pad=1 + (W * bpp) % 2, frame_gap=5, lead=FK.LEAD + 1, seed=seed)
        assert p.row_stride % 2 == 1 and p.offset(0) % 2 == 1
    return p


def device_annotate_records(det, fr, recs, counts, per_frame, st, stream=None):
    """det.annotate_records on a device copy of fr.buf -> the buffer afterwards"""
    import torch
    d = to_device(fr.buf)
    dm, dc = to_device(recs), to_device(np.asarray(counts, np.int32))
    torch.cuda.synchronize()
    det.annotate_records(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, dm.data_ptr(), dc.data_ptr(), per_frame=per_frame, style=st,
                         fmt=fr.fmt, row_stride=fr.row_stride, frame_stride=fr.frame_stride, stream=stream)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def placed_records(W, Hh, cam, slots=8):
    """[2, slots] posed records of a W x Hh frame and their counts: on the corners of the kernel's tiles (256 columns, 16 rows, a
    wave's 4 rows), on the frame's edges, partly and wholly outside, a bow-tie, an unmatched one; frame 1 holds one record"""
    places = [(min(AC.TILE_W, W - 1), min(AC.TILE_H, Hh - 1), 22, 30, 20), (0.0, 0.0, 18, 0, 70), (W - 1.0, Hh - 1.0, 30, 55, 200),
              (W * 0.5, AC.WAVE_ROWS - 0.5, 12, 40, 100), (W + 6.0, Hh * 0.4, 26, 20, 300), (-60.0, -60.0, 16, 0, 0)]
    recs = np.zeros((2, slots), FK.MARKER_DTYPE)
    for k, (u, v, size, tilt, gamma) in enumerate(places):
        R, t = PS.pose(cam, u, v, size, tilt, gamma, 30 + 50 * k)
        recs[0, k] = AC.posed_record(cam, R, t, template_id=[0, 7, 10, 4095, 123, 5][k], ratio=1.0 if k != 2 else 1.4)
    recs[0, 6] = FK.records([[W * 0.2, Hh * 0.2, W * 0.6, Hh * 0.9, W * 0.6, Hh * 0.2, W * 0.2, Hh * 0.9]], [31])[0]
    recs[0, 7] = FK.records([FK.axis_square(W // 3, Hh // 3, 9, 7)], [2], [0.0])[0]
    R, t = PS.pose(cam, W * 0.5, Hh * 0.5, min(W, Hh) * 0.6, 35, 45, 10)
    recs[1, 0] = AC.posed_record(cam, R, t, template_id=88)
    return recs, [8, 1]


def full_style(L, **kw):
    a = dict(flags=AC.ALL_FLAGS, thickness=2, axis_length=1.2, cube_height=0.9, outline=(30, 220, 90, 200), unmatched=(120, 120, 130, 255),
             corner0=(255, 40, 40, 160), cube=(20, 200, 230, 255), label=(250, 240, 30, 230))
    a.update(kw)
    return AC.style(L, **a)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("fmt", FK.FMTS)
@pytest.mark.parametrize("size", [(70, 37), (257, 17), (300, 33)])
def test_every_format_and_layout(oa, L, det320, size, fmt, aligned):
    W, Hh = size
    cam = cam_of(320, 240, True)
    fr = layout(2, W, Hh, fmt, aligned, seed=W)
    recs, counts = placed_records(W, Hh, cam)
    st = full_style(L)
    want, drawn = AC.host_annotate(L, fr, recs, counts, st, cam)
    assert drawn == [7, 1], drawn     # (the one wholly outside draws nothing)
    assert (want != fr.buf).any() and (want[~fr.pixel_mask()] == FK.GUARD).all()
    got = device_annotate_records(det320, fr, recs, counts, 8, st)
    same(got, want, fr, "%dx%d %s %s" % (W, Hh, fmt, "aligned" if aligned else "unaligned"))


def scattered(rng, n, W, Hh, lo, hi, cam, n_tids=4096):
    """n posed records of lo .. hi px, turned and tilted at random, all over (and over the edges of) a W x Hh frame; every fifth
    one unmatched"""
    recs = np.zeros(n, FK.MARKER_DTYPE)
    for k in range(n):
        R, t = PS.pose(cam, rng.uniform(-5, W + 5), rng.uniform(-5, Hh + 5), rng.uniform(lo, hi), rng.uniform(0, 60), rng.uniform(0, 360), rng.uniform(0, 360))
        recs[k] = AC.posed_record(cam, R, t, template_id=int(rng.integers(0, n_tids)), score=0.0 if k % 5 == 4 else 1.0)
    return recs


@pytest.mark.parametrize("stride", [1, 64, 65, 130])
def test_record_strides_and_counts(L, det320, stride):
    """counts 0, 1, the stride and above it, at strides on both sides of the 64 slots one ballot takes"""
    rng = np.random.default_rng(50 + stride)
    cam = cam_of(320, 240, True)
    fr = FK.Frames(4, 200, 120, "bgr", seed=stride)
    recs = np.stack([scattered(rng, stride, 200, 120, 8, 40, cam) for _ in range(4)])
    st = full_style(L, thickness=1)
    given = [0, 1, stride, stride + 7]
    want, drawn = AC.host_annotate(L, fr, recs, [0, 1, stride, stride], st, cam)
    assert drawn[0] == 0 and drawn[1] <= 1 and drawn[2] >= min(stride, 2) - 1 and drawn[3] >= min(stride, 2) - 1 and sum(drawn) >= 2
    got = device_annotate_records(det320, fr, recs, given, stride, st)
    same(got, want, fr, "stride %d" % stride)
    assert (fr.view(0, got) == fr.view(0)).all()


def test_overlapping_records_keep_their_order(L, det320):
    cam = cam_of(320, 240, True)
    sq = [FK.axis_square(20 + 9 * k, 15 + 4 * k, 60, 50) for k in range(6)]
    recs = FK.records(sq, [0, 1, 2, 3, 4, 5])[None]
    st = AC.style(L, AC.OUTLINE | AC.CORNER0 | AC.LABEL | AC.COLOR_BY_TEMPLATE, thickness=5, outline=(0, 0, 0, 150), label_scale=3,
                  label=(255, 255, 255, 140), corner0=(200, 0, 100, 99))
    fr = FK.Frames(1, 160, 100, "rgba", seed=3)
    want, _ = AC.host_annotate(L, fr, recs, [6], st, cam)
    backwards, _ = AC.host_annotate(L, fr, recs[:, ::-1].copy(), [6], st, cam)
    assert (want != backwards).any()     # the order shows
    same(device_annotate_records(det320, fr, recs, [6], 6, st), want, fr, "in order")
    same(device_annotate_records(det320, fr, recs[:, ::-1].copy(), [6], 6, st), backwards, fr, "backwards")


STYLES = [dict(flags=AC.OUTLINE), dict(flags=AC.CORNER0), dict(flags=AC.AXES), dict(flags=AC.CUBE), dict(flags=AC.LABEL),
          dict(flags=AC.OUTLINE | AC.UNMATCHED), dict(flags=AC.OUTLINE | AC.COLOR_BY_TEMPLATE), dict(flags=AC.ALL_FLAGS),
          dict(flags=AC.ALL_FLAGS, thickness=1, label_scale=1), dict(flags=AC.ALL_FLAGS, thickness=16, label_scale=8),
          dict(flags=AC.ALL_FLAGS, thickness=16, label_scale=1, axis_length=0.0, cube_height=0.0),
          dict(flags=AC.DRAW_FLAGS, thickness=3, outline=(1, 2, 3, 0), cube=(9, 9, 9, 0))]


@pytest.mark.parametrize("case", range(len(STYLES)))
def test_flags_thicknesses_and_label_scales(L, det320, case):
    cam = cam_of(320, 240, True)
    W, Hh = 300, 33
    fr = layout(2, W, Hh, "bgr" if case % 2 else "gray", case % 3 != 0, seed=case)
    recs, counts = placed_records(W, Hh, cam)
    st = full_style(L, **STYLES[case])
    want, drawn = AC.host_annotate(L, fr, recs, counts, st, cam)
    assert sum(drawn) >= 2 and (want != fr.buf).any()
    same(device_annotate_records(det320, fr, recs, counts, 8, st), want, fr, str(STYLES[case]))


def test_more_frames_than_the_context_holds_go_in_chunks(oa, L):
    det = oa.Detector(64, 64, max_batch=2)
    cam = cam_of(64, 48, False)
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    rng = np.random.default_rng(70)
    fr = FK.Frames(5, 64, 48, "rgb", row_pad=4, seed=70)
    recs = np.stack([scattered(rng, 64, 64, 48, 8, 30, cam) for _ in range(5)])
    counts = [3, 0, 64, 7, 1]
    st = full_style(L)
    want, drawn = AC.host_annotate(L, fr, recs, counts, st, cam)
    assert drawn[1] == 0 and min(drawn[0], drawn[2], drawn[3]) >= 1
    same(device_annotate_records(det, fr, recs, counts, 64, st), want, fr, "chunks")


def test_on_a_stream_of_the_caller(oa, L, det320):
    import torch
    cam = cam_of(320, 240, True)
    fr = layout(2, 257, 17, "bgra", True, seed=8)
    recs, counts = placed_records(257, 17, cam)
    st = full_style(L)
    want, _ = AC.host_annotate(L, fr, recs, counts, st, cam)
    s = torch.cuda.Stream()
    same(device_annotate_records(det320, fr, recs, counts, 8, st, stream=s.cuda_stream), want, fr, "caller's stream")
    # two calls on two streams back to back: the library orders them on its workspace
    d = to_device(fr.buf)
    dm, dc = to_device(recs), to_device(np.asarray(counts, np.int32))
    torch.cuda.synchronize()
    for stream in (s.cuda_stream, None):
        det320.annotate_records(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, dm.data_ptr(), dc.data_ptr(), per_frame=8, style=st,
                                fmt=fr.fmt, row_stride=fr.row_stride, frame_stride=fr.frame_stride, stream=stream)
        torch.cuda.synchronize()
    twice, _ = AC.host_annotate(L, fr, recs, counts, st, cam, buf=want)
    same(d.cpu().numpy(), twice, fr, "twice")


# ---- bound to a batch ---------------------------------------------------------------------------------------------------------

TPL = 2   # 4x4-01: decodes in every rotation
COLOUR = np.array([250, 10, 200, 180], np.uint8)   # R G B A


@pytest.fixture(scope="module")
def batch():
    """four 320 x 240 views of one marker each"""
    scenes = [PS.scene("annotate", "g%d" % g, 320, 240, [(150 + 5 * k, 120, 90, 15 * k, g, 40, TPL, None)]) for k, g in enumerate((10, 100, 190, 280))]
    fr = FK.Frames(4, 320, 240, "bgr")
    for f, s in enumerate(scenes):
        fr.view(f)[...] = s.frame
    return dict(scenes=scenes, fr=fr, cam=scenes[0].cam)


def batch_detector(oa, b, overlay=False, gate=None):
    det = oa.Detector(320, 240, max_batch=4)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates([PS.NAMES[TPL]])])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(b["cam"])))
    if overlay:
        det.set_overlay(-1, np.broadcast_to(COLOUR, (4, 4, 4)).copy())
    if gate is not None:
        det.set_gate(gate)
    return det


def detect_and_annotate(det, fr, st, render=False, stream=None):
    """enqueue on the frames, (render and) annotate into a clone, collect -> (the clone's buffer, markers, counts)"""
    import torch
    d = to_device(fr.buf)
    clone = d.clone()
    torch.cuda.synchronize()
    det.enqueue_device(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    if render:
        det.render(clone.data_ptr() + fr.offset(0), fr.width, fr.height, row_stride=fr.row_stride, frame_stride=fr.frame_stride, stream=stream)
    det.annotate(clone.data_ptr() + fr.offset(0), fr.width, fr.height, style=st, row_stride=fr.row_stride, frame_stride=fr.frame_stride, stream=stream)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == fr.buf).all()   # the detected frames themselves are untouched
    return clone.cpu().numpy(), markers, counts


def test_annotate_between_enqueue_and_collect(oa, L, LO, batch):
    fr, cam = batch["fr"], batch["cam"]
    st = full_style(L)
    got, markers, counts = detect_and_annotate(batch_detector(oa, batch), fr, st)
    assert counts.tolist() == [1, 1, 1, 1] and (markers[:, 0]["score"] > 0).all()
    want, drawn = AC.host_annotate(L, fr, markers, counts, st, cam)
    assert drawn == [1, 1, 1, 1]
    same(got, want, fr, "bound to the batch")
    # markers and counts do not depend on the call
    d = to_device(fr.buf)
    plain, pcounts = batch_detector(oa, batch).detect_device(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n)
    assert plain.tobytes() == markers.tobytes() and (pcounts == counts).all()
    # render, then annotate, on one batch: the host overlay followed by the host annotate
    both, m2, c2 = detect_and_annotate(batch_detector(oa, batch, overlay=True), fr, st, render=True)
    assert m2.tobytes() == markers.tobytes() and (c2 == counts).all()
    under, _ = OC.host_render(LO, fr, markers, counts, {-1: np.broadcast_to(COLOUR, (4, 4, 4)).copy()})
    want2, _ = AC.host_annotate(L, fr, markers, counts, st, cam, buf=under)
    assert (want2 != want).any()
    same(both, want2, fr, "render, then annotate")


def test_under_a_gate_and_on_a_stream_of_the_caller(oa, L, batch):
    import torch
    fr, cam = batch["fr"], batch["cam"]
    st = full_style(L, thickness=3)
    gate = oa.Gate(width=2)
    det = batch_detector(oa, batch, gate=gate)
    got, markers, counts = detect_and_annotate(det, fr, st)
    want, _ = AC.host_annotate(L, fr, markers, counts, st, cam)
    same(got, want, fr, "gate: annotate against the host core")
    later = device_annotate_records(det, fr, markers, counts, det.max_markers, st)
    same(later, want, fr, "gate: annotate_records afterwards")
    s = torch.cuda.Stream()
    got2, m2, c2 = detect_and_annotate(det, fr, st, stream=s.cuda_stream)
    assert m2.tobytes() == markers.tobytes()
    same(got2, want, fr, "gate: on the caller's stream")
    det.close()


def test_a_context_that_never_annotates_allocates_nothing(oa, L, batch):
    """device memory in use: a context that detects and renders records but never annotates holds what it held before those
    calls; the first annotate call of a context takes its workspace (so the counter would have shown one).  The figure is the
    whole device's, so a difference is looked at again on a fresh context: another process's allocation does not repeat."""
    import torch
    fr = batch["fr"]
    recs = FK.records([FK.axis_square(10, 10, 40, 40)] * 4).reshape(4, 1)
    d, dm, dc = to_device(fr.buf), to_device(recs), to_device(np.ones(4, np.int32))
    st = AC.style(L, AC.OUTLINE)

    def annotate(det):
        det.annotate_records(d.data_ptr() + fr.offset(0), 320, 240, 4, dm.data_ptr(), dc.data_ptr(), per_frame=1, style=st)
        torch.cuda.synchronize()

    annotate(oa.Detector(320, 240, max_batch=4))     # (the process's first launches load the code object)
    for attempt in range(3):
        det = batch_detector(oa, batch, overlay=True)
        det.detect_device(d.data_ptr() + fr.offset(0), 320, 240, 4)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        det.detect_device(d.data_ptr() + fr.offset(0), 320, 240, 4)
        det.render_records(d.data_ptr() + fr.offset(0), 320, 240, 4, dm.data_ptr(), dc.data_ptr(), per_frame=1)
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        if after == before:
            break
    assert after == before, (before, after)
    # 512 frames x 64 slots x 696 bytes = 22 MB: no allocation granularity hides it
    ws = 512 * 64 * oa.ANNO_RECORD_BYTES
    d16, dm16, dc16 = to_device(np.zeros(16 * 16 * 3, np.uint8)), to_device(recs[:1]), to_device(np.ones(1, np.int32))
    for attempt in range(3):
        big = oa.Detector(16, 16, max_batch=512)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        big.annotate_records(d16.data_ptr(), 16, 16, 1, dm16.data_ptr(), dc16.data_ptr(), per_frame=1, style=st)
        torch.cuda.synchronize()
        first = before - torch.cuda.mem_get_info()[0]
        big.annotate_records(d16.data_ptr(), 16, 16, 1, dm16.data_ptr(), dc16.data_ptr(), per_frame=1, style=st)
        torch.cuda.synchronize()
        second = before - torch.cuda.mem_get_info()[0]
        if first >= 0.9 * ws and second - first < ws // 2:
            break
    assert first >= 0.9 * ws and second - first < ws // 2, (first, second)   # the first call takes the workspace, the second nothing


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_frames_alone(oa, L, batch):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(320, 240, max_batch=4)
    ctx = det._ctx
    W, Hh = 320, 240
    frames = np.full((4, Hh, W, 3), 200, np.uint8)
    d = to_device(frames)
    recs = to_device(FK.records([FK.axis_square(5, 5, 50, 50)] * 4).reshape(4, 1))
    cnt = to_device(np.ones(4, np.int32))
    torch.cuda.synchronize()
    fp, rp, cp = d.data_ptr(), recs.data_ptr(), cnt.data_ptr()
    good = AC.style(L, AC.OUTLINE | AC.LABEL)
    sp = C.addressof(good)

    def records(**kw):
        a = dict(fp=fp, w=W, h=Hh, rs=3 * W, n=4, fmt=0, rp=rp, cp=cp, per=1, sp=sp)
        a.update(kw)
        return lib.ocvar_hip_annotate_records(ctx, a["fp"], a["w"], a["h"], a["rs"], a["rs"] * a["h"], a["n"], a["fmt"], a["rp"], a["cp"], a["per"],
                                              a["sp"], None)

    def bound(c, **kw):
        a = dict(fp=fp, w=W, h=Hh, rs=3 * W, fmt=0, sp=sp)
        a.update(kw)
        return lib.ocvar_hip_annotate(c, a["fp"], a["w"], a["h"], a["rs"], a["rs"] * a["h"], a["fmt"], a["sp"], None)

    # sizes, strides, formats, pointers: as render_records refuses them
    M = det.max_markers
    for kw in [dict(per=0), dict(per=M + 1), dict(n=0), dict(fmt=5), dict(fmt=-1), dict(rs=3 * W - 1), dict(w=321), dict(h=241), dict(w=0),
               dict(fp=None), dict(rp=None), dict(cp=None), dict(sp=None)]:
        assert records(**kw) == E_ARG, kw
    # a bad style
    bad_styles = [dict(thickness=0), dict(thickness=17), dict(label_scale=-1), dict(label_scale=9), dict(axis_length=-1.0),
                  dict(cube_height=float("nan")), dict(axis_length=float("inf")), dict(flags=128 | 1), dict(flags=0), dict(flags=AC.UNMATCHED)]
    for kw in bad_styles:
        s = AC.style(L, **kw)
        assert records(sp=C.addressof(s)) == E_ARG, kw
    # AXES and CUBE without a camera
    for flags in (AC.AXES, AC.CUBE, AC.ALL_FLAGS):
        s = AC.style(L, flags)
        assert records(sp=C.addressof(s)) == E_ARG, flags
    # bound to a batch: nothing enqueued
    assert bound(ctx) == E_ARG and b"nothing enqueued" in lib.ocvar_hip_last_error(ctx)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates()])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
    det.enqueue_device(fp, W, Hh, 4)
    for kw in [dict(w=319), dict(h=239), dict(fmt=5), dict(rs=3 * W - 1), dict(fmt=2, rs=4 * W - 1), dict(fp=None), dict(sp=None)]:
        assert bound(ctx, **kw) == E_ARG, kw
    for kw in bad_styles:
        s = AC.style(L, **kw)
        assert bound(ctx, sp=C.addressof(s)) == E_ARG, kw
    det.collect()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == frames.reshape(-1)).all()
    # and after all that the context still draws, axes included now that it has a camera
    s = AC.style(L, AC.ALL_FLAGS)
    assert records(sp=C.addressof(s)) == 0 and records() == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() != frames.reshape(-1)).any()

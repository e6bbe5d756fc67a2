"""Overlays on the device (ocvar_hip_set_overlay / ocvar_hip_render / ocvar_hip_render_records) byte for byte against the host
build of overlay_core.h (tests/overlay_chain.py): whole buffers are compared, the guard bytes in the row padding, between the
frames and around the buffer included."""
import ctypes as C

import numpy as np
import pytest

import dense_synth as DS
import frame_kit as FK
import helpers as H
import overlay_chain as OC
import persp_synth as PS
from frame_kit import E_ARG, oa, same, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

SET5 = (5, 30, 0.1)


@pytest.fixture(scope="module")
def L():
    return OC.build_emul()


@pytest.fixture(scope="module")
def overlays():
    rng = np.random.default_rng(41)
    return {0: OC.random_overlay(rng, 2, 2), 1: OC.random_overlay(rng, 3, 5), 2: OC.random_overlay(rng, 64, 64),
            3: OC.random_overlay(rng, 257, 129)}


@pytest.fixture(scope="module")
def det320(oa, overlays):
    det = oa.Detector(320, 240, max_batch=4)
    for t, o in overlays.items():
        det.set_overlay(t, o)
    return det


def device_render_records(det, fr, recs, counts, per_frame, buf=None):
    """det.render_records on a device copy of fr.buf (or buf) -> the buffer afterwards"""
    import torch
    d = to_device(fr.buf if buf is None else buf)
    dm, dc = to_device(recs), to_device(np.asarray(counts, np.int32))
    torch.cuda.synchronize()
    det.render_records(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, dm.data_ptr(), dc.data_ptr(), per_frame=per_frame,
                       fmt=fr.fmt, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def six_records(W, Hh):
    """the kinds of record a kernel can get wrong: an overlapping pair, one cut by a corner of the frame, one wholly outside, a
    degenerate one, one that covers the whole frame (frame 2, count 6), and one smaller than a pixel (frame 1, count 1)"""
    cx, cy, s = W * 0.45, Hh * 0.5, min(W, Hh) * 0.3
    pair_a = [cx - s, cy - s * 0.8, cx + s * 0.9, cy - s, cx + s, cy + s * 0.7, cx - s * 0.8, cy + s]
    pair_b = [cx, cy - s * 0.5, cx + s * 1.2, cy + s * 0.1, cx + s * 0.4, cy + s * 1.1, cx - s * 0.6, cy + s * 0.5]
    corner = [W - 9.5, Hh - 7.25, W + 11, Hh - 4, W + 8, Hh + 12, W - 6, Hh + 9]
    outside = [-40, -30, -20, -30, -20, -10, -40, -10]
    degenerate = [3, 3, 9, 9, 15, 15, 21, 21]
    whole = [-3, -2, W + 2, -3, W + 3, Hh + 2, -2, Hh + 3]
    tiny = [9.75, 9.8, 10.3, 9.75, 10.35, 10.3, 9.8, 10.25]
    recs = np.zeros((3, 8), FK.MARKER_DTYPE)
    recs[1, :1] = FK.records([tiny], [1])
    recs[2, :6] = FK.records([whole, pair_a, pair_b, corner, outside, degenerate], [0, 2, 3, 1, 2, 3])
    return recs, [0, 1, 6]


@pytest.mark.parametrize("row_pad", [0, 5])
@pytest.mark.parametrize("fmt", ["bgr", "rgb", "bgra", "rgba", "gray"])
@pytest.mark.parametrize("size", [(61, 37), (64, 64), (257, 131)])
def test_render_records_on_hand_made_records(L, det320, overlays, size, fmt, row_pad):
    W, Hh = size
    fr = FK.Frames(3, W, Hh, fmt, row_pad=row_pad, frame_gap=12, seed=W + row_pad)
    recs, counts = six_records(W, Hh)
    want, drawn = OC.host_render(L, fr, recs, counts, overlays)
    assert drawn == [0, 1, 4]   # (outside and degenerate draw nothing)
    assert (want != fr.buf).any() and (want[~fr.pixel_mask()] == FK.GUARD).all()
    got = device_render_records(det320, fr, recs, counts, 8)
    same(got, want, fr, "%dx%d %s pad %d" % (W, Hh, fmt, row_pad))


def scattered(rng, n, W, Hh, lo, hi, n_tids):
    """n random squares of lo .. hi px side, turned at random, all over (and over the edges of) a W x Hh frame"""
    sq = np.zeros((n, 4, 2), np.float32)
    for k in range(n):
        s, a = rng.uniform(lo, hi), rng.uniform(0, 2 * np.pi)
        c = np.array([rng.uniform(-5, W + 5), rng.uniform(-5, Hh + 5)])
        ang = a + np.arange(4) * np.pi / 2
        sq[k] = c + s / np.sqrt(2) * np.stack([np.cos(ang), np.sin(ang)], 1)
    return FK.records(sq, rng.integers(0, n_tids, n))


@pytest.mark.parametrize("stride", [1, 8, 64])
def test_record_strides_and_counts_above_the_stride(L, det320, overlays, stride):
    rng = np.random.default_rng(50 + stride)
    fr = FK.Frames(2, 200, 120, "bgr", row_pad=0, seed=stride)
    recs = np.stack([scattered(rng, stride, 200, 120, 10, 60, 4) for _ in range(2)])
    given = [stride + 5, 10 ** 6]          # read as the stride
    want, drawn = OC.host_render(L, fr, recs, [stride, stride], overlays)
    assert min(drawn) >= 1
    got = device_render_records(det320, fr, recs, given, stride)
    same(got, want, fr, "stride %d" % stride)


def test_dense_context_walks_its_list_beyond_64(oa, L, overlays):
    det = oa.Detector(320, 240, max_batch=1, max_markers=512)
    assert det.max_markers == 512
    for t, o in overlays.items():
        det.set_overlay(t if t else -1, o)   # (the 2 x 2 one as the default overlay)
    rng = np.random.default_rng(60)
    fr = FK.Frames(1, 320, 240, "rgba", seed=60)
    recs = scattered(rng, 512, 320, 240, 4, 40, 6)[None]
    ovs = {(t if t else -1): o for t, o in overlays.items()}
    want, drawn = OC.host_render(L, fr, recs, [512], ovs)
    assert drawn[0] > 400
    got = device_render_records(det, fr, recs, [512], 512)
    same(got, want, fr, "dense")


def test_more_frames_than_the_context_holds_go_in_chunks(oa, L, overlays):
    det = oa.Detector(64, 64, max_batch=2)
    det.set_overlay(-1, overlays[2])
    rng = np.random.default_rng(70)
    fr = FK.Frames(5, 64, 48, "rgb", row_pad=4, seed=70)
    recs = np.stack([scattered(rng, 64, 64, 48, 8, 30, 1) for _ in range(5)])
    counts = [3, 0, 64, 7, 1]
    want, drawn = OC.host_render(L, fr, recs, counts, {-1: overlays[2]})
    assert drawn[1] == 0 and min(drawn[0], drawn[2], drawn[3], drawn[4]) >= 1
    got = device_render_records(det, fr, recs, counts, 64)
    same(got, want, fr, "chunks")


# ---- end to end -------------------------------------------------------------------------------------------------------------

N_E2E = 4
COLOUR = np.array([250, 10, 200, 255], np.uint8)   # R G B A


@pytest.fixture(scope="module")
def e2e():
    """four frames of synth_config(3) (1080p, 16 markers), every marker with a template of its own -- the registration keeps one
    marker per template, so that is what it takes for all sixteen to have a record"""
    cfg = H.synth_config(3)
    names = DS.library(16, size=4, seed=31)
    frames, truth = zip(*[H.synth_frame(cfg, f, names) for f in range(N_E2E)])
    # (the generator's pixel (x, y) covers [x, x + 1): pixel centres at integers are half a pixel less)
    quads = [[t["corner"] - 0.5 for t in tr] for tr in truth]
    return dict(cfg=cfg, frames=np.stack(frames), quads=quads, tpls=H.oracle_templates(names), cam=H.oracle_camera(cfg.width, cfg.height))


def e2e_detector(oa, sc, refine=None, overlay=True, gate=None):
    det = oa.Detector(sc["cfg"].width, sc["cfg"].height, max_batch=N_E2E)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in sc["tpls"]])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(sc["cam"])))
    if refine:
        det.set_corner_refine(*refine)
    if overlay:
        det.set_overlay(-1, np.broadcast_to(COLOUR, (4, 4, 4)).copy())
    if gate is not None:
        det.set_gate(gate)
    return det


def frames_of(sc):
    fr = FK.Frames(N_E2E, sc["cfg"].width, sc["cfg"].height, "bgr")
    for f in range(N_E2E):
        fr.view(f)[...] = sc["frames"][f]
    return fr


def detect_and_render(det, fr):
    """enqueue on the frames, render into a clone, collect -> (rendered buffer, markers, counts)"""
    import torch
    d = to_device(fr.buf)
    clone = d.clone()
    torch.cuda.synchronize()
    det.enqueue_device(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    det.render(clone.data_ptr() + fr.offset(0), fr.width, fr.height, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == fr.buf).all()   # the detected frames themselves are untouched
    return clone.cpu().numpy(), markers, counts


@pytest.mark.parametrize("refine", [None, SET5])
def test_end_to_end_render_between_enqueue_and_collect(oa, L, e2e, refine):
    sc = e2e
    fr = frames_of(sc)
    got, markers, counts = detect_and_render(e2e_detector(oa, sc, refine), fr)
    want, drawn = OC.host_render(L, fr, markers, counts, {-1: np.broadcast_to(COLOUR, (4, 4, 4)).copy()})
    assert min(drawn) == 16, drawn
    same(got, want, fr, "end to end")
    bgr = COLOUR[[2, 1, 0]]
    for f in range(N_E2E):
        img = fr.view(f, got)
        margin = np.max([OC.inside_quad(q, fr.width, fr.height) for q in sc["quads"][f]], axis=0)   # > 0 inside some truth quad
        inside, outside = margin >= 2, margin < -2
        assert inside.sum() > 16 * 100 * 100
        assert (img[inside] == bgr).all(), (f, int((img[inside] != bgr).any(axis=1).sum()))
        assert (img[outside] == sc["frames"][f][outside]).all(), f
    plain, pcounts = None, None
    det0 = e2e_detector(oa, sc, refine, overlay=False)
    d = to_device(fr.buf)
    plain, pcounts = det0.detect_device(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, row_stride=fr.row_stride,
                                        frame_stride=fr.frame_stride)
    assert plain.tobytes() == markers.tobytes() and (pcounts == counts).all()


def test_render_under_a_gate_equals_render_records_afterwards(oa, L, e2e):
    import torch
    sc = e2e
    fr = frames_of(sc)
    gate = oa.Gate(width=2)
    det = e2e_detector(oa, sc, gate=gate)
    got, markers, counts = detect_and_render(det, fr)
    assert int(counts.min()) == 16
    later = device_render_records(det, fr, markers, counts, det.max_markers)
    same(got, later, fr, "gate: render against render_records")
    want, _ = OC.host_render(L, fr, markers, counts, {-1: np.broadcast_to(COLOUR, (4, 4, 4)).copy()})
    same(got, want, fr, "gate: render against the host core")
    det.close()


def test_the_overlay_follows_the_marker_not_the_frame(oa, e2e):
    """One marker at its four in-plane rotations, an overlay with a mark at its top-left texels.  Decoded at orient 1, 2 or 4 the
    mark lies at the marker's corner 0 -- the template image's bottom-left corner, the projection of persp_synth.OBJ[0] -- wherever
    that is in the frame; at orient 3 (turned by 180 degrees) at the opposite corner, as include/ocvar_hip.h says."""
    import torch
    tpl = 2   # 4x4-01: decodes in every rotation
    scenes = [PS.scene("turn", "g%d" % g, 640, 480, [(320, 240, 160, 0, g, 0, tpl, None)]) for g in (10, 100, 190, 280)]
    det = oa.Detector(640, 480, max_batch=4)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates([PS.NAMES[tpl]])])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(scenes[0].cam)))
    ov = np.zeros((32, 32, 4), np.uint8)
    ov[...] = (90, 90, 90, 255)
    ov[:12, :12] = (255, 0, 0, 255)
    det.set_overlay(0, ov)
    d = to_device(np.stack([s.frame for s in scenes]))
    torch.cuda.synchronize()
    det.enqueue_device(d.data_ptr(), 640, 480, 4)
    det.render(d.data_ptr(), 640, 480)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    out = d.cpu().numpy().reshape(4, 480, 640, 3)
    seen = []
    for f, s in enumerate(scenes):
        assert counts[f] == 1 and markers[f, 0]["score"] > 0
        q = s.markers[0].quad
        centre = q.mean(axis=0)
        red = []
        for c in range(4):
            x, y = np.rint(centre + 0.75 * (q[c] - centre)).astype(int)
            px = out[f, y, x]
            assert tuple(px) in ((0, 0, 255), (90, 90, 90)), (f, c, px)
            red.append(tuple(px) == (0, 0, 255))
        assert sum(red) == 1
        seen.append((red.index(True), tuple(np.rint(q[red.index(True)]).astype(int))))
    assert [c for c, _ in seen] == [0, 0, 2, 0], seen          # (190 degrees decodes at orient 3)
    assert len({p for c, p in seen if c == 0}) == 3, seen      # three different places in the frame: it follows the marker


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_frames_alone(oa, overlays):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(320, 240, max_batch=2)
    ctx = det._ctx
    img = np.ascontiguousarray(overlays[2])
    p = C.c_void_p(img.ctypes.data)
    W, Hh = 320, 240
    frames = np.full((2, Hh, W, 3), 200, np.uint8)
    d = to_device(frames)
    recs = to_device(FK.records([FK.axis_square(5, 5, 50, 50)] * 2).reshape(2, 1))
    cnt = to_device(np.array([1, 1], np.int32))
    torch.cuda.synchronize()
    fp, rp, cp = d.data_ptr(), recs.data_ptr(), cnt.data_ptr()

    # nothing set yet: no overlay
    assert lib.ocvar_hip_render_records(ctx, fp, W, Hh, 3 * W, 3 * W * Hh, 2, 0, rp, cp, 1, None) == E_ARG
    for w, h, rs, tid in [(1, 64, 256, 0), (1025, 64, 4100, 0), (64, 1, 256, 0), (64, 1025, 256, 0), (64, 64, 255, 0), (64, 64, 256, -2),
                          (64, 64, 256, 4096)]:
        assert lib.ocvar_hip_set_overlay(ctx, tid, p, w, h, rs) == E_ARG, (w, h, rs, tid)
    for t in range(63):
        assert lib.ocvar_hip_set_overlay(ctx, t, p, 2, 2, 256) == 0
    assert lib.ocvar_hip_set_overlay(ctx, -1, p, 2, 2, 256) == 0
    assert lib.ocvar_hip_set_overlay(ctx, 100, p, 2, 2, 256) == E_ARG     # the 65th
    assert lib.ocvar_hip_set_overlay(ctx, 5, p, 64, 64, 256) == 0         # replacing one is not a 65th
    assert lib.ocvar_hip_set_overlay(ctx, 7, None, 0, 0, 0) == 0 and lib.ocvar_hip_set_overlay(ctx, 100, p, 2, 2, 256) == 0

    M = det.max_markers
    bad_records = [dict(per=0), dict(per=M + 1), dict(n=0), dict(fmt=5), dict(fmt=-1), dict(rs=3 * W - 1), dict(w=321), dict(h=241),
                   dict(w=0), dict(fp=None), dict(rp=None), dict(cp=None)]
    for kw in bad_records:
        a = dict(fp=fp, w=W, h=Hh, rs=3 * W, n=2, fmt=0, rp=rp, cp=cp, per=1)
        a.update(kw)
        rc = lib.ocvar_hip_render_records(ctx, a["fp"], a["w"], a["h"], a["rs"], a["rs"] * a["h"], a["n"], a["fmt"], a["rp"], a["cp"],
                                          a["per"], None)
        assert rc == E_ARG, kw
    # render: nothing enqueued
    assert lib.ocvar_hip_render(ctx, fp, W, Hh, 3 * W, 3 * W * Hh, 0, None) == E_ARG
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates()])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
    det.enqueue_device(fp, W, Hh, 2)
    for kw in [dict(w=319), dict(h=239), dict(fmt=5), dict(rs=3 * W - 1), dict(fmt=2, rs=4 * W - 1), dict(fp=None)]:
        a = dict(fp=fp, w=W, h=Hh, rs=3 * W, fmt=0)
        a.update(kw)
        assert lib.ocvar_hip_render(ctx, a["fp"], a["w"], a["h"], a["rs"], a["rs"] * a["h"], a["fmt"], None) == E_ARG, kw
    assert lib.ocvar_hip_set_overlay(ctx, 9, p, 64, 64, 256) == E_ARG     # a batch is in flight
    assert lib.ocvar_hip_set_overlay(ctx, 9, None, 0, 0, 0) == E_ARG
    det.collect()
    # a context without overlays refuses render
    det2 = oa.Detector(320, 240, max_batch=2)
    det2.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates()])
    det2.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
    det2.enqueue_device(fp, W, Hh, 2)
    assert lib.ocvar_hip_render(det2._ctx, fp, W, Hh, 3 * W, 3 * W * Hh, 0, None) == E_ARG
    det2.collect()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == frames.reshape(-1)).all()
    # and after all that the context still draws
    assert lib.ocvar_hip_render_records(ctx, fp, W, Hh, 3 * W, 3 * W * Hh, 2, 0, rp, cp, 1, None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() != frames.reshape(-1)).any()

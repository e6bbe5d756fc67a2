"""Patches on the device (ocvar_hip_patches / ocvar_hip_patches_records) byte for byte against the host build of patch_core.h
(tests/patch_chain.py): whole patch buffers are compared, the guard bytes around the block and the slots that are not written
included, and every status."""

import numpy as np
import pytest

import frame_kit as FK
import helpers as H
import overlay_chain as OC
import patch_chain as PC
from frame_kit import E_ARG, FMTS, oa, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

SET5 = (5, 30, 0.1)
FRAME_SIZES = [(61, 37), (64, 64), (257, 131)]
PATCH_SIZES = [s for s in PC.SIZES if s != (16, 16)]


@pytest.fixture(scope="module")
def L():
    return PC.build_emul()


@pytest.fixture(scope="module")
def LO():
    return OC.build_emul()


@pytest.fixture(scope="module")
def det320(oa):
    return oa.Detector(320, 240, max_batch=2)


def device_patches_records(det, fr, recs, counts, pt, flags=0, with_status=True, buf=None):
    """det.patches_records on device copies of fr.buf (or buf) and of the guard-filled pt.buf -> (patch buffer, status [n, slots] or
    None, the frame buffer afterwards)"""
    import torch
    d = to_device(fr.buf if buf is None else buf)
    dp = to_device(pt.buf)
    dm, dc = to_device(np.ascontiguousarray(recs)), to_device(np.asarray(counts, np.int32))
    ds = to_device(np.full((fr.n, pt.slots), PC.STATUS_FILL, np.int32)) if with_status else None
    torch.cuda.synchronize()
    det.patches_records(d.data_ptr() + fr.offset(0), fr.width, fr.height, fr.n, dm.data_ptr(), dc.data_ptr(), dp.data_ptr() + pt.lead,
                        pt.pw, pt.ph, per_frame=pt.slots, fmt=fr.fmt, row_stride=fr.row_stride, frame_stride=fr.frame_stride,
                        flip_rows=bool(flags & PC.FLIP_ROWS), matched_only=bool(flags & PC.MATCHED_ONLY),
                        d_status_ptr=ds.data_ptr() if with_status else None)
    torch.cuda.synchronize()
    status = ds.cpu().numpy().view(np.int32).reshape(fr.n, pt.slots) if with_status else None
    return dp.cpu().numpy(), status, d.cpu().numpy()


def same(got, want, pt, where):
    bad = np.flatnonzero(got != want)
    if bad.size:
        inside = (bad >= pt.lead) & (bad < got.size - FK.LEAD)
        slot = (bad[0] - pt.lead) // pt.slot_bytes
        raise AssertionError("%s: %d bytes differ (%d of them outside the block), first at %d (frame %d slot %d byte %d): %d != %d" % (
            where, bad.size, int((~inside).sum()), bad[0], slot // pt.slots, slot % pt.slots, (bad[0] - pt.lead) % pt.slot_bytes,
            got[bad[0]], want[bad[0]]))


def hand_made_records(W, Hh):
    """the kinds of record a kernel can get wrong -- one that covers the whole frame, an overlapping pair, one cut by a corner of
    the frame, one wholly outside, a degenerate one -- and the status cases: a NaN, an inf and a 2e6 coordinate, score 0 (frame 2,
    count 10); one smaller than a pixel (frame 1, count 1, with live records behind the count); nothing (frame 0)"""
    cx, cy, s = W * 0.45, Hh * 0.5, min(W, Hh) * 0.3
    pair_a = [cx - s, cy - s * 0.8, cx + s * 0.9, cy - s, cx + s, cy + s * 0.7, cx - s * 0.8, cy + s]
    pair_b = [cx, cy - s * 0.5, cx + s * 1.2, cy + s * 0.1, cx + s * 0.4, cy + s * 1.1, cx - s * 0.6, cy + s * 0.5]
    corner = [W - 9.5, Hh - 7.25, W + 11, Hh - 4, W + 8, Hh + 12, W - 6, Hh + 9]
    outside = [-40, -30, -20, -30, -20, -10, -40, -10]
    degenerate = [3, 3, 9, 9, 15, 15, 21, 21]
    whole = [-3, -2, W + 2, -3, W + 3, Hh + 2, -2, Hh + 3]
    tiny = [9.75, 9.8, 10.3, 9.75, 10.35, 10.3, 9.8, 10.25]
    nan, inf, far = list(pair_a), list(pair_b), list(whole)
    nan[7], inf[0], far[2] = np.nan, np.inf, -2e6
    recs = np.zeros((3, 12), FK.MARKER_DTYPE)
    recs[0, :2] = FK.records([pair_a, pair_b])
    recs[1, :3] = FK.records([tiny, pair_a, whole])
    recs[2, :10] = FK.records([whole, pair_a, pair_b, corner, outside, degenerate, nan, inf, far, pair_b], scores=[1, 1, 1, 1, 1, 1, 1, 1, 1, 0])
    plain = [[0] * 12, [1] + [0] * 11, [1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0]]
    matched = [[0] * 12, [1] + [0] * 11, [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]]
    return recs, [0, 1, 10], plain, matched


# every frame size, row padding and patch size with every format, without the full product
HAND_MADE = [(fmt, FRAME_SIZES[(i + j) % 3], 5 * ((i + j) % 2), PATCH_SIZES[i], (i + j) % 4) for j, fmt in enumerate(FMTS) for i in range(len(PATCH_SIZES))]


def test_the_hand_made_cases_cover_every_value_with_every_format():
    for fmt in FMTS:
        mine = [c for c in HAND_MADE if c[0] == fmt]
        assert {c[1] for c in mine} == set(FRAME_SIZES) and {c[2] for c in mine} == {0, 5} and {c[3] for c in mine} == set(PATCH_SIZES)


@pytest.mark.parametrize("fmt,size,row_pad,patch,flags", HAND_MADE)
def test_patches_records_on_hand_made_records(L, det320, fmt, size, row_pad, patch, flags):
    W, Hh = size
    pw, ph = patch
    fr = FK.Frames(3, W, Hh, fmt, row_pad=row_pad, frame_gap=12, seed=W + row_pad)
    recs, counts, plain, matched = hand_made_records(W, Hh)
    pt, want, want_status = PC.host_patches(L, fr, recs, counts, pw, ph, flags)
    assert (want_status == (matched if flags & PC.MATCHED_ONLY else plain)).all()
    v = pt.view(want)
    assert (v[want_status == 0] == FK.GUARD).all() and (v[2, 4] == 0).all() and (v[2, 0] != v[2, 1]).any()
    got, status, frames_after = device_patches_records(det320, fr, recs, counts, pt, flags)
    assert (frames_after == fr.buf).all()
    assert (status == want_status).all(), status.tolist()
    same(got, want, pt, "%dx%d %s pad %d patch %dx%d flags %d" % (W, Hh, fmt, row_pad, pw, ph, flags))


def scattered(rng, n, W, Hh):
    return FK.records(PC.random_quads(rng, n, W, Hh), scores=rng.integers(0, 2, n))


@pytest.mark.parametrize("stride,flags,with_status", [(1, PC.FLIP_ROWS, True), (8, PC.MATCHED_ONLY, False), (64, PC.FLIP_ROWS | PC.MATCHED_ONLY, True)])
@pytest.mark.parametrize("fmt,patch", [("gray", (16, 16)), ("bgr", (63, 17)), ("rgba", (3, 5))])
def test_strides_chunks_an_odd_address_and_no_status(L, det320, stride, flags, with_status, fmt, patch):
    """three frames on a context of two; counts above the stride are read as it; the patch block at an odd byte address"""
    rng = np.random.default_rng(50 + stride)
    fr = FK.Frames(3, 200, 120, fmt, row_pad=1, seed=stride)
    recs = np.stack([scattered(rng, stride, 200, 120) for _ in range(3)])
    given = [stride + 5, 10 ** 6, stride - 1 if stride > 1 else 1]
    pt, want, want_status = PC.host_patches(L, fr, recs, np.minimum(given, stride), patch[0], patch[1], flags, lead=FK.LEAD + 1)
    assert want_status.sum() >= 1
    got, status, _ = device_patches_records(det320, fr, recs, given, pt, flags, with_status=with_status)
    if with_status:
        assert (status == want_status).all()
    same(got, want, pt, "stride %d %s" % (stride, fmt))


def test_an_aligned_block_of_whole_dwords_next_to_an_unaligned_one(L, det320):
    """the same records into a block whose address and slot size are multiples of 4 (dword stores) and into one a byte further"""
    rng = np.random.default_rng(77)
    for fmt, (pw, ph) in (("gray", (64, 64)), ("bgr", (20, 7)), ("bgra", (65, 33)), ("gray", (66, 5))):   # (66 x 5: a tail of 2 px)
        fr = FK.Frames(2, 257, 131, fmt, seed=3)
        recs = np.stack([scattered(rng, 8, 257, 131) for _ in range(2)])
        for lead in (FK.LEAD, FK.LEAD + 1, FK.LEAD + 2):
            pt, want, want_status = PC.host_patches(L, fr, recs, [8, 6], pw, ph, 0, lead=lead)
            got, status, _ = device_patches_records(det320, fr, recs, [8, 6], pt)
            assert (status == want_status).all()
            same(got, want, pt, "%s %dx%d lead %d" % (fmt, pw, ph, lead))


# ---- between enqueue and collect ----------------------------------------------------------------------------------------------

N_E2E, PER = 4, 4
PW, PH = 48, 40
COLOUR = np.array([250, 10, 200, 255], np.uint8)   # R G B A


@pytest.fixture(scope="module")
def e2e():
    """four synthetic 320 x 240 frames with two or three markers each, and the oracle's records for them"""
    cfg = H.synth_config(2, width=320, height=240, side_min=48, side_max=72)
    frames = np.stack([H.synth_frame(cfg, f)[0] for f in range(N_E2E)])
    tpls, cam = H.oracle_templates(), H.oracle_camera(cfg.width, cfg.height)
    refs = [H.oracle_registration(frames[f], tpls, cam) for f in range(N_E2E)]
    assert all(2 <= len(r[0]) <= PER for r in refs)
    return dict(cfg=cfg, frames=frames, tpls=tpls, cam=cam, refs=refs)


def e2e_detector(oa, sc, refine=None, gate=None, overlay=False):
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


def enqueue_and_patch(det, fr, pt, grey_in_place=False, render=False, flags=0):
    """enqueue on the frames, (render,) patches, collect -> (patch buffer, status, markers, counts, the frames afterwards)"""
    import torch
    d, dp = to_device(fr.buf), to_device(pt.buf)
    ds = to_device(np.full((fr.n, pt.slots), PC.STATUS_FILL, np.int32))
    torch.cuda.synchronize()
    fp = d.data_ptr() + fr.offset(0)
    det.enqueue_device(fp, fr.width, fr.height, fr.n, row_stride=fr.row_stride, frame_stride=fr.frame_stride, grey_in_place=grey_in_place)
    if render:
        det.render(fp, fr.width, fr.height, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    det.patches(fp, fr.width, fr.height, dp.data_ptr() + pt.lead, pt.pw, pt.ph, per_frame=pt.slots, row_stride=fr.row_stride,
                frame_stride=fr.frame_stride, flip_rows=bool(flags & PC.FLIP_ROWS), matched_only=bool(flags & PC.MATCHED_ONLY),
                d_status_ptr=ds.data_ptr())
    markers, counts = det.collect()
    torch.cuda.synchronize()
    return dp.cpu().numpy(), ds.cpu().numpy().view(np.int32).reshape(fr.n, pt.slots), markers, counts, d.cpu().numpy()


def check_against_host(L, fr, pt, got, status, markers, counts, frames_then, flags, where):
    _, want, want_status = PC.host_patches(L, fr, markers, counts, pt.pw, pt.ph, flags, per_frame=pt.slots, buf=frames_then)
    assert (status == want_status).all(), (where, status.tolist(), want_status.tolist())
    assert want_status.sum() == int(np.minimum(counts, pt.slots).sum()) >= 2 * N_E2E
    same(got, want, pt, where)


@pytest.mark.parametrize("grey_in_place", [False, True])
def test_patches_between_enqueue_and_collect_against_host_build_and_oracle(oa, L, e2e, grey_in_place):
    sc, fr = e2e, frames_of(e2e)
    pt = PC.Patches(N_E2E, PER, PW, PH, 3)
    got, status, markers, counts, then = enqueue_and_patch(e2e_detector(oa, sc), fr, pt, grey_in_place=grey_in_place)
    for f in range(N_E2E):   # the frames as they are then: greyed by the batch, or untouched
        assert (fr.view(f, then) == (sc["refs"][f][2] if grey_in_place else sc["frames"][f])).all()
    check_against_host(L, fr, pt, got, status, markers, counts, then, 0, "grey_in_place %s" % grey_in_place)
    # the oracle chain on the oracle's own records and (greyed) frames
    v = pt.view(got)
    for f in range(N_E2E):
        ref_markers, _, grey = sc["refs"][f]
        img = grey if grey_in_place else sc["frames"][f]
        planes = [np.ascontiguousarray(img[..., c]) for c in range(3)]
        assert counts[f] == len(ref_markers)
        for k, r in enumerate(ref_markers):
            sq = np.array(r.square, np.float32)
            assert (markers[f, k]["square"] == sq).all(), (f, k)
            mc, mo = PC.core_map32(L, sq, PW, PH), PC.oracle_map32(sq, PW, PH)
            want = PC.oracle_warp(planes, mo if mc.tobytes() == mo.tobytes() else mc, PW, PH)
            assert (v[f, k] == want).all(), (f, k, int((v[f, k] != want).sum()))
            assert want.min() < 100 and want.max() > 150   # (a marker: black and white)


def test_patches_of_refined_corners(oa, L, e2e):
    sc, fr = e2e, frames_of(e2e)
    pt = PC.Patches(N_E2E, PER, PW, PH, 3)
    got, status, markers, counts, then = enqueue_and_patch(e2e_detector(oa, sc, refine=SET5), fr, pt, flags=PC.FLIP_ROWS | PC.MATCHED_ONLY)
    assert any((markers[f, k]["square"] != np.array(r.square, np.float32)).any() for f in range(N_E2E) for k, r in enumerate(sc["refs"][f][0]))
    check_against_host(L, fr, pt, got, status, markers, counts, then, PC.FLIP_ROWS | PC.MATCHED_ONLY, "refined")


def test_patches_on_contexts_of_a_gate_with_fewer_lanes(oa, L, e2e):
    import torch
    sc, fr = e2e, frames_of(e2e)
    gate = oa.Gate(width=2, lanes=2)
    dets = [e2e_detector(oa, sc, gate=gate) for _ in range(3)]
    pt = PC.Patches(N_E2E, PER, PW, PH, 3)
    d = to_device(fr.buf)
    dps = [to_device(pt.buf) for _ in dets]
    dss = [to_device(np.full((fr.n, pt.slots), PC.STATUS_FILL, np.int32)) for _ in dets]
    torch.cuda.synchronize()
    fp = d.data_ptr() + fr.offset(0)
    for det in dets:
        det.enqueue_device(fp, fr.width, fr.height, fr.n, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    for det, dp, ds in zip(dets, dps, dss):
        det.patches(fp, fr.width, fr.height, dp.data_ptr() + pt.lead, PW, PH, per_frame=PER, row_stride=fr.row_stride,
                    frame_stride=fr.frame_stride, d_status_ptr=ds.data_ptr())
    for i in (1, 2, 0):
        markers, counts = dets[i].collect()
        # (collect on a context of a gate has waited for the patches as well: no synchronise in between)
        got = dps[i].cpu().numpy()
        status = dss[i].cpu().numpy().view(np.int32).reshape(fr.n, pt.slots)
        check_against_host(L, fr, pt, got, status, markers, counts, fr.buf, 0, "gate, context %d" % i)
    torch.cuda.synchronize()
    for det in dets:
        det.close()


def test_patches_after_render_show_the_overlay(oa, L, LO, e2e):
    sc, fr = e2e, frames_of(e2e)
    pt = PC.Patches(N_E2E, PER, PW, PH, 3)
    got, status, markers, counts, then = enqueue_and_patch(e2e_detector(oa, sc, overlay=True), fr, pt, render=True)
    rendered, drawn = OC.host_render(LO, fr, markers, counts, {-1: np.broadcast_to(COLOUR, (4, 4, 4)).copy()})
    assert min(drawn) >= 2 and (then == rendered).all()
    check_against_host(L, fr, pt, got, status, markers, counts, rendered, 0, "after render")
    v = pt.view(got)
    for f in range(N_E2E):
        for k in range(int(counts[f])):
            assert (v[f, k, 4:-4, 4:-4] == COLOUR[[2, 1, 0]]).all(), (f, k)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(oa):
    import torch
    lib = oa.hip_lib()
    det = oa.Detector(320, 240, max_batch=2)
    ctx = det._ctx
    W, Hh, M = 320, 240, det.max_markers
    d = to_device(np.full((2, Hh, W, 3), 200, np.uint8))
    recs = to_device(FK.records([FK.axis_square(5, 5, 50, 50)] * 2).reshape(2, 1))
    cnt = to_device(np.array([1, 1], np.int32))
    out = np.full(2 * 256 * 256 * 4 + 64, FK.GUARD, np.uint8)
    dp = to_device(out)
    ds = to_device(np.full(2 * M, PC.STATUS_FILL, np.int32))
    torch.cuda.synchronize()
    fp, rp, cp, pp, sp = d.data_ptr(), recs.data_ptr(), cnt.data_ptr(), dp.data_ptr(), ds.data_ptr()

    def records_call(**kw):
        a = dict(fp=fp, w=W, h=Hh, rs=3 * W, n=2, fmt=0, rp=rp, cp=cp, per=1, pp=pp, pw=16, ph=16, flags=0)
        a.update(kw)
        return lib.ocvar_hip_patches_records(ctx, a["fp"], a["w"], a["h"], a["rs"], a["rs"] * a["h"], a["n"], a["fmt"], a["rp"], a["cp"],
                                             a["per"], a["pp"], a["pw"], a["ph"], a["flags"], sp, None)

    def batch_call(c, **kw):
        a = dict(fp=fp, w=W, h=Hh, rs=3 * W, fmt=0, pp=pp, pw=16, ph=16, per=1, flags=0)
        a.update(kw)
        return lib.ocvar_hip_patches(c, a["fp"], a["w"], a["h"], a["rs"], a["rs"] * a["h"], a["fmt"], a["pp"], a["pw"], a["ph"], a["per"],
                                     a["flags"], sp, None)

    common = [dict(fp=None), dict(pp=None), dict(fmt=5), dict(fmt=-1), dict(rs=3 * W - 1), dict(fmt=2, rs=4 * W - 1), dict(pw=1), dict(ph=1),
              dict(pw=257), dict(ph=257), dict(flags=4), dict(flags=-1), dict(per=0), dict(per=M + 1)]
    for kw in common + [dict(n=0), dict(w=321), dict(h=241), dict(w=0), dict(rp=None), dict(cp=None)]:
        assert records_call(**kw) == E_ARG, kw
        assert lib.ocvar_hip_last_error(ctx), kw
    assert batch_call(ctx) == E_ARG   # nothing enqueued
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates()])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
    det.enqueue_device(fp, W, Hh, 2)
    for kw in common + [dict(w=319), dict(h=239)]:
        assert batch_call(ctx, **kw) == E_ARG, kw
    det.collect()
    assert batch_call(ctx) == E_ARG   # collected: nothing enqueued again
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == out).all() and (ds.cpu().numpy().view(np.int32) == PC.STATUS_FILL).all()
    # and after all that the context still extracts
    assert records_call() == 0
    torch.cuda.synchronize()
    got = dp.cpu().numpy()
    assert (got[:2 * 16 * 16 * 3] == 200).all() and (got[2 * 16 * 16 * 3:] == FK.GUARD).all()
    assert (ds.cpu().numpy().view(np.int32)[:2] == 1).all()

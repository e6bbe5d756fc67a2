"""Frames at the size and stride limits the C ABI admits (include/ocvar_hip.h: contexts of 16 .. 32767 pixels each way, any
row_stride the frame kernel can address), against the oracle under the bars of tests/test_gpu_parity.py: grey plane, binary
image, every bit of the mask plane, frame quads, candidates, marker ids / scores / squares bit-exact, glMatrix within 1e-4
relative -- no marker left out, and no frame let off with OCVAR_E_CAPACITY.

What the sizes are for (the bounds live in comments of hd.h / binarise.hip; tests/test_geometry_limits_cpu.py checks the
arithmetic itself on the CPU): corner points travel packed as x | y << 16; the row division div14; 24-bit tile offsets; the
137 panels of a 32767-wide grey plane; scan positions y * ns + x beyond 2^24 (ns = 32768 from row 512 on); and source rows read
through a buffer resource of 2^31 - 1 bytes, which api.hip now refuses to exceed (hd.h::frame_src_addressable)."""
import ctypes as C

import numpy as np
import pytest

import frame_kit as FK
import geometry_scenes as GS
import helpers as H
import overlay_chain as OC
import refine_chain as RC
from frame_kit import E_ARG, FMTS, GUARD, oa  # noqa: F401
from test_gpu_input_formats import as_format, grey_in_place_of
from test_gpu_parity import OracleFrame, check_candidates, check_markers, check_planes

pytestmark = pytest.mark.gpu

E_CAPACITY = -4
INT_MAX = 2**31 - 1
SET5 = (5, 30, 0.1)
GUARD_BYTES = 64


def detector(oa, w, h, tpls, cam, batch=1):
    det = oa.Detector(w, h, max_batch=batch)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    return det


def flags(oa, det):
    return oa.hip_lib().ocvar_hip_capacity_flags(det._ctx)


def check_all(oa, det, ref, markers, counts, where):
    assert flags(oa, det) == 0, where
    check_planes(det, 0, ref, where)
    check_candidates(det, 0, ref, where)
    check_markers(0, ref, markers, counts, where)
    assert markers.shape[1] >= len(ref.markers)   # (check_markers compared every record)


_long = {}


def long_scene(tall):
    """the 32767 x 600 (600 x 32767) frame of geometry_scenes.long_frame and the oracle's results on it, made once"""
    if tall not in _long:
        frame, regions = GS.long_frame(tall)
        h, w = frame.shape[:2]
        tpls, cam = H.oracle_templates(GS.LIBRARY), GS.pinhole_camera(w, h)
        _long[tall] = dict(frame=frame, regions=regions, w=w, h=h, tpls=tpls, cam=cam, ref=OracleFrame(frame, tpls, cam))
    return _long[tall]


@pytest.mark.parametrize("tall", [False, True], ids=["32767x600", "600x32767"])
def test_long_frames_with_scenes_at_the_origin_the_centre_and_the_far_corner(oa, tall):
    """32767 x 600 and 600 x 32767: the full width (height) a context can have, and from row 512 on scan positions beyond 2^24 in
    the word they share with the hole flag.  Scenes at the origin, at the centre and flush with the far corner, each with templates
    of its own so that markers of all three survive the elimination; a strip of markers the far edge cuts.  Everything against
    the oracle; records (poses included) whose four corners all lie beyond 32000; a decoded candidate of the cut strip; the
    caller's frame greyed in place; and on the wide frame the square finder alone on the grey image."""
    sc = long_scene(tall)
    w, h, ref = sc["w"], sc["h"], sc["ref"]
    det = detector(oa, w, h, sc["tpls"], sc["cam"])
    frames = sc["frame"][None].copy()
    markers, counts = det.detect_host(frames, grey_in_place=True)
    check_all(oa, det, ref, markers, counts, ("long", tall))
    assert np.array_equal(frames[0], np.broadcast_to(ref.grey[..., None], frames[0].shape))   # greyed in place as the oracle does
    axis = 1 if tall else 0
    far = [k for k in range(counts[0]) if (markers[0, k]["square"].reshape(4, 2)[:, axis] >= 32000).all()]
    assert len(far) >= 3, far                                # (their ids, squares and poses were compared above)
    assert len(ref.cands) >= 100 and counts[0] >= 6
    cut = [c for c in det.debug_candidates(0) if c.orient and GS.inside(c.square, sc["regions"]["cut"])]
    assert len(cut) >= 2                                     # the strip the far edge cuts through still gives decoded candidates
    assert (np.array([c.square for c in cut]).reshape(-1, 4, 2)[:, :, axis] >= 32000).all()
    if not tall:
        got, n = det.find_squares(ref.grey)
        assert n == len(ref.quads) and np.array_equal(got, ref.quads)
        assert (ref.quads[:, :, 0].min(axis=1) >= 32000).sum() >= 8


@pytest.mark.parametrize("w,h", [(32767, 16), (16, 32767), (32767, 33), (33, 32767)])
def test_one_strip_or_one_chunk_at_the_full_length(oa, w, h):
    """The thinnest frames at the full length: 16 pixels are one strip (one chunk) and the byte-wise loads of images narrower
    than 32 columns; 33 adds the odd last row or column to the full length of the other side.  Random 4 x 4 blocks: no marker
    fits, every border rule is at work over 137 panels or 2341 tile rows."""
    frame = GS.block_frame(w, h, w + h)
    tpls, cam = H.oracle_templates(), GS.pinhole_camera(w, h)
    det = detector(oa, w, h, tpls, cam)
    markers, counts = det.detect_host(frame[None].copy())
    check_all(oa, det, OracleFrame(frame, tpls, cam), markers, counts, (w, h))


def test_odd_last_column_that_begins_the_last_grey_panel(oa):
    """32641 x 64: column 32640 = 136 * 240 begins grey panel 136 and is the odd last column (greyed by its own kernel, stored
    twice) -- test_odd_sizes_whose_last_column_or_row_begins_a_grey_panel at the last panel a plane can have; textured, with
    34 small markers along the frame whose crops read across panel seams."""
    w, h = 32641, 64
    cfg = H.synth_config(3, textured=1, width=w, height=h, grid_x=w // 960, grid_y=1, side_min=30, side_max=36)
    frame, _ = H.synth_frame(cfg, 0)
    tpls, cam = H.oracle_templates(), GS.pinhole_camera(w, h)
    det = detector(oa, w, h, tpls, cam)
    markers, counts = det.detect_host(frame[None].copy())
    ref = OracleFrame(frame, tpls, cam)
    check_all(oa, det, ref, markers, counts, (w, h))
    assert len(ref.cands) >= 90 and counts[0] >= 2
    assert max(np.array(c.square).reshape(4, 2)[:, 0].max() for c in ref.cands) >= 32400


def test_one_marker_2500_pixels_on_its_side(oa):
    """One 4x4 marker 2500 px on its side, turned 20 degrees, in a 4096 x 4096 grey frame (2^24 scan positions): its borders'
    squared bounding-box diagonals are ~2 * 10^7, far above 2^21, where the followers order borders by 64-bit keys, and its
    outer border has 6816 corner points.  The result must be the oracle's -- or, if a border does not fit the followers' slabs
    and pool, the call must fail with OCVAR_E_CAPACITY and flags within 2 | 8 (point pool, trace overrun): loud, not wrong.
    Observed on an MI355X: the first of the two -- the frame is handled and equals the oracle (one marker, six candidates);
    no capacity flag is raised."""
    import torch
    size = 4096
    grey = GS.big_marker_frame(size)
    bgr = np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=2))
    tpls, cam = H.oracle_templates(), H.oracle_camera(size, size)
    det = detector(oa, size, size, tpls, cam)
    det.set_input_format("gray")
    d = torch.from_numpy(grey).cuda()
    try:
        markers, counts = det.detect_device(d.data_ptr(), size, size, 1)
    except oa.OcvarError as e:
        f = flags(oa, det)
        print("big marker: OCVAR_E_CAPACITY, flags", f)
        assert "(%d)" % E_CAPACITY in str(e), str(e)
        assert f != 0 and f & ~(2 | 8) == 0, f
        return
    print("big marker: handled, %d markers" % counts[0])
    ref = OracleFrame(bgr, tpls, cam)
    check_all(oa, det, ref, markers, counts, "big marker")
    assert counts[0] == 1
    sq = markers[0, 0]["square"].reshape(4, 2)
    assert ((sq.max(0) - sq.min(0)) ** 2).sum() > 2**21 * 8


def test_opt_in_stages_at_far_coordinates(oa):
    """Corner refinement (5 / 30 / 0.1) and the overlay renderer on the 32767 x 600 scene, whose records reach x = 32690:
    refined squares bit-exact against the host chain of tests/refine_chain.py (poses within the bar), and the frame rendered
    with a default overlay byte for byte against tests/overlay_chain.py's host renderer, guard bytes included."""
    import torch
    sc = long_scene(False)
    w, h, ref = sc["w"], sc["h"], sc["ref"]
    Lr = RC.build_emul()
    Lo = OC.build_emul()
    overlay = OC.random_overlay(np.random.default_rng(9), 16, 16)
    det = detector(oa, w, h, sc["tpls"], sc["cam"])
    det.set_corner_refine(*SET5)
    det.set_overlay(-1, overlay)
    fr = FK.Frames(1, w, h, "bgr", row_pad=5, fill=0)
    fr.view(0)[...] = sc["frame"]
    d = torch.from_numpy(fr.buf).cuda()
    clone = d.clone()
    torch.cuda.synchronize()
    det.enqueue_device(d.data_ptr() + fr.offset(0), w, h, 1, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    det.render(clone.data_ptr() + fr.offset(0), w, h, row_stride=fr.row_stride, frame_stride=fr.frame_stride)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    assert flags(oa, det) == 0
    exp = RC.refined_markers(Lr, ref.markers, ref.grey, sc["cam"], SET5)
    RC.check(markers, counts, 0, exp, "far refine")
    moved = sum(not np.array_equal(np.array(a.square), np.array(b.square)) for a, b in zip(exp, ref.markers))
    assert moved >= 4                                        # the refinement does move these corners: the comparison is not vacuous
    want, drawn = OC.host_render(Lo, fr, markers, counts, {-1: overlay})
    assert drawn[0] >= 6, (drawn, counts)
    got = clone.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    changed = np.flatnonzero((fr.view(0, got) != sc["frame"]).any(axis=(0, 2)))
    assert changed.min() < 640 and changed.max() >= 32000    # drawn at both ends of the frame
    assert np.array_equal(d.cpu().numpy(), fr.buf)           # the detected frames themselves are untouched


# ---- rows that span 2 GiB ------------------------------------------------------------------------------------------------

_small = {}


def small_scene(fmt):
    """the 320 x 240 frame with its markers in the bottom 100 rows, in fmt, and the oracle on the BGR frame of the same colours
    (the colour formats share one)"""
    key = "gray" if fmt == "gray" else "colour"
    bgr0, _ = GS.bottom_rows_frame(1)
    src, bgr = as_format(bgr0, fmt, 77)
    if key not in _small:
        tpls, cam = H.oracle_templates(), H.oracle_camera(320, 240)
        ref = OracleFrame(bgr, tpls, cam)
        assert len(ref.cands) >= 9 and len(ref.markers) >= 1
        assert all(np.array(c.square).reshape(4, 2)[:, 1].min() >= 140 for c in ref.cands)
        _small[key] = (tpls, cam, ref)
    return (src,) + _small[key]


def largest_stride(bpp, w=320, h=240):
    """the largest row_stride include/ocvar_hip.h's rule accepts for a w x h frame of bpp bytes per pixel"""
    return (INT_MAX - bpp * (w & ~1)) // ((h & ~1) - 1)


class Spread:
    """rows of a frame `stride` bytes apart in an otherwise unwritten device buffer, each followed by GUARD_BYTES guard bytes"""

    def __init__(self, src, stride, buffer_bytes):
        import torch
        h = src.shape[0]
        self.row = src.reshape(h, -1)
        self.h, self.n = h, self.row.shape[1]
        assert (h - 1) * stride + self.n + GUARD_BYTES <= buffer_bytes
        self.buf = torch.empty(buffer_bytes, dtype=torch.uint8, device="cuda")
        self.rows = torch.as_strided(self.buf, (h, self.n + GUARD_BYTES), (stride, 1))
        self.written = np.concatenate([self.row, np.full((h, GUARD_BYTES), GUARD, np.uint8)], axis=1)
        self.rows.copy_(torch.from_numpy(self.written))
        torch.cuda.synchronize()

    def read(self):
        return self.rows.cpu().numpy()

    def free(self):
        import torch
        self.rows = self.buf = None
        torch.cuda.empty_cache()


def raw_enqueue(oa, det, ptr, stride, frame_stride):
    lib = oa.hip_lib()
    rc = lib.ocvar_hip_enqueue(det._ctx, ptr, 320, 240, stride, frame_stride, 1, 1, None, None, None)
    return rc, lib.ocvar_hip_last_error(det._ctx).decode()


@pytest.mark.parametrize("fmt", FMTS)
def test_largest_row_span_the_rule_accepts(oa, fmt):
    """320 x 240 with the largest row_stride the rule accepts, in a device buffer of 2 GiB + slack of which only the 240 rows and
    64 guard bytes behind each are written: row 239 ends on the last byte the frame kernel's 2^31 - 1 byte resource covers, and
    all markers lie in the bottom 100 rows.  Results equal the oracle, the rows come back greyed, the guards are untouched."""
    src, tpls, cam, ref = small_scene(fmt)
    bpp = FK.bpp_of(fmt)
    stride = largest_stride(bpp)
    assert 239 * stride + bpp * 320 <= INT_MAX < 239 * (stride + 1) + bpp * 320
    assert 140 * stride > INT_MAX - 100 * stride             # the marker rows begin in the last 100 strides below 2^31
    sp = Spread(src, stride, (1 << 31) + 4096)
    try:
        det = detector(oa, 320, 240, tpls, cam)
        det.set_input_format(fmt)
        markers, counts = det.detect_device(sp.buf.data_ptr(), 320, 240, 1, row_stride=stride, grey_in_place=True)
        check_all(oa, det, ref, markers, counts, (fmt, stride))
        out = sp.read()
        want = grey_in_place_of(src, fmt, ref.grey).reshape(240, -1)
        assert np.array_equal(out[:, :sp.n], want)
        assert (out[:, sp.n:] == GUARD).all()
    finally:
        sp.free()


@pytest.mark.parametrize("fmt", FMTS)
def test_one_byte_more_of_row_stride_is_refused(oa, fmt):
    """row_stride one byte above the largest accepted: OCVAR_E_ARG with a text, nothing enqueued, the buffer -- row 239 and the
    guards included -- unchanged although grey_in_place was asked for; a legal call on the same context afterwards is right."""
    import torch
    src, tpls, cam, ref = small_scene(fmt)
    stride = largest_stride(FK.bpp_of(fmt)) + 1
    sp = Spread(src, stride, (1 << 31) + 4096)
    try:
        det = detector(oa, 320, 240, tpls, cam)
        det.set_input_format(fmt)
        rc, text = raw_enqueue(oa, det, sp.buf.data_ptr(), stride, 240 * stride)
        assert rc == E_ARG and "2147483647" in text and "row_stride" in text, (rc, text)
        torch.cuda.synchronize()
        assert np.array_equal(sp.read(), sp.written)
        assert oa.hip_lib().ocvar_hip_ready(det._ctx) < 0        # nothing is enqueued
        d = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        markers, counts = det.detect_device(d.data_ptr(), 320, 240, 1)
        check_all(oa, det, ref, markers, counts, (fmt, "after the refusal"))
    finally:
        sp.free()


@pytest.mark.parametrize("fmt", FMTS)
def test_row_239_beyond_4_gib_is_refused(oa, fmt):
    """a row_stride that puts row 239 beyond 2^32 bytes (its offset wrapped to 32 bits would look like a small, legal one), in a
    buffer of 4 GiB + slack: OCVAR_E_ARG, the buffer unchanged"""
    import torch
    src, tpls, cam, ref = small_scene(fmt)
    stride = 2**32 // 239 + 1
    assert stride <= INT_MAX and 239 * stride >= 2**32
    sp = Spread(src, stride, (1 << 32) + 8192)
    try:
        det = detector(oa, 320, 240, tpls, cam)
        det.set_input_format(fmt)
        rc, text = raw_enqueue(oa, det, sp.buf.data_ptr(), stride, 240 * stride)
        assert rc == E_ARG and "2147483647" in text, (rc, text)
        torch.cuda.synchronize()
        assert np.array_equal(sp.read(), sp.written)
    finally:
        sp.free()


def test_host_frames_inherit_the_refusal(oa):
    """ocvar_hip_detect_host stages the caller's frames at the caller's strides, so the same rule holds for host frames: refused
    before anything is staged (the pointer is never read: a 1-byte array stands in for a 2 GiB frame), and the context takes
    the next call."""
    lib = oa.hip_lib()
    tpls, cam = H.oracle_templates(), H.oracle_camera(320, 240)
    det = detector(oa, 320, 240, tpls, cam)
    stride = largest_stride(3) + 1
    one = np.zeros(1, np.uint8)
    counts = np.zeros(1, np.int32)
    markers = np.zeros(64, oa.MARKER_DTYPE)
    rc = lib.ocvar_hip_detect_host(det._ctx, one.ctypes.data, 320, 240, stride, 240 * stride, 1, 0, None, None, markers.ctypes.data,
                                   counts.ctypes.data, 64)
    assert rc == E_ARG and "2147483647" in lib.ocvar_hip_last_error(det._ctx).decode()
    src, _, _, ref = small_scene("bgr")
    m, c = det.detect_host(np.ascontiguousarray(src[None]))
    check_all(oa, det, ref, m, c, "host call after the refusal")

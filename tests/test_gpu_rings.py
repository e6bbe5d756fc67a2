"""GPU tests of the verdicts of follow.hip::ring_quads_kernel, read back with ocvar_hip_debug_rings: for every frame and every crop
of a batch the flag must be 1 exactly when both sides of the plane are at least 8 and the ring next to its zeroed 1-px frame --
rows 1 and sh-2, columns 1 and sw-2 -- is all set in the binary image the same batch wrote (debug_binary / debug_crop_binary).
The scenes (tests/ring_scenes.py; tests/test_rings_cpu.py proves from the oracle what each holds) put a hole at every place where
the kernel's masks, lanes, rounds and trips change, mix crop shapes within every group of 64, and take both grid-stride loops a
second time.  The planes themselves are compared with the oracle's, and the candidates and markers of every distinct frame too:
a ring wrongly called clean loses the border that begins at (1, 1)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import ring_scenes as R
from frame_kit import oa  # noqa: F401
from test_gpu_parity import OracleFrame, check_candidates, check_markers, check_planes, make_detector
from test_gpu_starts import size

pytestmark = pytest.mark.gpu


def crop_plane(det, r):
    """debug_crop_binary of record r of det.debug_crops(), without reading the ROI list again for every crop"""
    out = np.zeros((int(r["h"]) & -2, int(r["w"]) & -2), np.uint8)
    rc = det._lib.ocvar_hip_debug_crop_plane(det._ctx, int(r["index"]), 0, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, ("ocvar_hip_debug_crop_plane", rc, [int(v) for v in r])
    return out


def check_flag(flag, binary, what):
    """one verdict against the rule on the plane it was made from; a mismatch names the ROI, its geometry and the first hole"""
    want = R.rule(binary)
    if int(flag) != want:
        sh, sw = binary.shape
        holes = R.cleared(binary)
        raise AssertionError(("ring verdict", what, "flag", int(flag), "rule", want, "ns, sh, sw", (R.plane_stride(sw), sh, sw),
                              "items", R.ring_items(sw, sh)[1], "first cleared ring pixel", holes[0] if holes else None))
    return want


def check_rings(det, n_frames, W, Hh, where, refs=None, crop_planes_of=None):
    """the flags of every frame and every crop of det's last batch against the rule; with refs (batch position -> OracleFrame
    with planes) every crop plane of those frames against the oracle's binarise of the oracle's grey crop -- of the positions in
    crop_planes_of every crop, of the others every 50th.  Returns (frame verdicts, crop records, crop verdicts)"""
    ff = det.debug_rings(False)
    assert ff.dtype == np.int32 and len(ff) == n_frames, (where, len(ff))
    frame_verdicts = [check_flag(ff[f], det.debug_binary(f, W, Hh), (where, "frame", f)) for f in range(n_frames)]
    rois = det.debug_crops()
    cf = det.debug_rings(True)
    assert len(cf) == len(rois) == int(det.counters()[1]), (where, len(cf), len(rois), det.counters().tolist())
    crop_verdicts = []
    for k, r in enumerate(rois):
        assert int(r["index"]) == k
        b = crop_plane(det, r)
        crop_verdicts.append(check_flag(cf[k], b, (where, "crop", [int(v) for v in r])))
        f = int(r["frame"])
        if refs is not None and f in refs and (crop_planes_of is None or f in crop_planes_of or k % 50 == 0):
            x0, y0, w, h = (int(r[n]) for n in ("x0", "y0", "w", "h"))
            want = H.oracle_binarise(refs[f].grey[y0:y0 + h, x0:x0 + w])
            assert np.array_equal(b[1:-1, 1:-1], want[1:-1, 1:-1]), ("crop plane", where, [int(v) for v in r])
            assert not b[0].any() and not b[-1].any() and not b[:, 0].any() and not b[:, -1].any(), ("crop frame", where, k)
    return np.array(frame_verdicts), rois, np.array(crop_verdicts)


def oracle_refs(grey_frames, W, Hh):
    """distinct grey frame (its bytes) -> OracleFrame with planes, computed once"""
    tpls, cam = H.oracle_templates(), H.oracle_camera(W, Hh)
    cache = {}

    def get(g):
        key = g.tobytes()
        if key not in cache:
            cache[key] = OracleFrame(R.bgr(g), tpls, cam)
        return cache[key]
    return get


def check_results(det, f, ref, markers, counts, where):
    check_planes(det, f, ref, where)
    check_candidates(det, f, ref, where)
    check_markers(f, ref, markers, counts, where)


@pytest.mark.parametrize("W,Hh", [(98, 67), (320, 240), (96, 520)])
def test_frame_rings_by_hole_position(oa, W, Hh):
    """one clean frame and one frame per hole position: corners, tile seams, last_bit, tile-row seams, lane and trip seams"""
    frames, names, where = R.frame_scene(W, Hh)
    n = len(frames)
    assert n > 8
    get = oracle_refs(frames, W, Hh)
    det, _, _ = make_detector(oa, size(W, Hh), None, n)
    markers, counts = det.detect_host(np.stack([R.bgr(g) for g in frames]))
    refs = {f: get(frames[f]) for f in range(n)}
    verdicts, rois, _ = check_rings(det, n, W, Hh, (W, Hh), refs)
    assert verdicts.tolist() == [1] + [0] * (n - 1), [(nm, p) for nm, p, v in zip(names, where, verdicts) if v != (p is None)]
    assert len(rois) >= n   # (every frame has a square, so the crop pass ran on all of them)
    for f in range(n):
        check_results(det, f, refs[f], markers, counts, (W, Hh, names[f]))
    det.close()


def test_crop_rings_by_shape_and_hole_position(oa):
    """ten frames that each hold every shape of crop -- the four parities, clipped by each frame edge, more than 256 ring items --
    with holes of every kind cycled over them: every group of 64 ROIs mixes ns, sh and sw"""
    frames, plan = R.crop_scene()
    n = len(frames)
    get = oracle_refs(frames, R.CW, R.CH)
    det, _, _ = make_detector(oa, size(R.CW, R.CH), None, n)
    markers, counts = det.detect_host(np.stack([R.bgr(g) for g in frames]))
    refs = {f: get(frames[f]) for f in range(n)}
    verdicts, rois, crop_verdicts = check_rings(det, n, R.CW, R.CH, "crop scene", refs)
    # (a dot on the ring of a crop that a frame edge clips opens the frame's own ring too)
    assert verdicts.tolist() == [R.rule(refs[f].binary) for f in range(n)] and 0 < verdicts.sum() < n
    assert len(rois) == sum(len(rows) for rows in plan) > 128
    # the verdicts are the oracle's, crop by crop
    for f in range(n):
        want = {c[:4]: int(not c[4]) for c in R.crop_rings(frames[f])}
        got = {tuple(int(r[k]) for k in ("x0", "y0", "w", "h")): int(v) for r, v in zip(rois, crop_verdicts) if int(r["frame"]) == f}
        assert got == want, (f, sorted(set(got.items()) ^ set(want.items())))
    groups = [{(R.plane_stride(int(r["w"]) & ~1), int(r["h"]) & ~1, int(r["w"]) & ~1) for r in rois[k:k + 64]} for k in range(0, len(rois), 64)]
    assert all(len(g) >= 2 for g in groups), groups
    for f in range(n):
        check_results(det, f, refs[f], markers, counts, ("crop scene", f))
    det.close()


def test_frame_rings_of_more_than_4096_frames(oa):
    """4100 frames in one batch from device memory (the host entry cuts a call into batches of 64): frames 4096 .. 4099 are the
    second trip of ring_quads_kernel<false>'s grid-stride loop"""
    import torch
    distinct, index = R.stride_scene()
    W, Hh, n = R.STRIDE_W, R.STRIDE_H, len(index)
    get = oracle_refs(distinct, W, Hh)
    det, _, _ = make_detector(oa, size(W, Hh), None, n)
    d = torch.from_numpy(np.stack([R.bgr(g) for g in distinct])[index]).cuda()
    torch.cuda.synchronize()
    markers, counts = det.detect_device(d.data_ptr(), W, Hh, n)
    verdicts, _, _ = check_rings(det, n, W, Hh, "4100 frames")
    assert verdicts.tolist() == [int(f % 3 != 2) for f in range(n)]
    first = {int(k): f for f, k in reversed(list(enumerate(index)))}
    for f in sorted(set(first.values()) | set(range(4096, n))):
        check_results(det, f, get(distinct[index[f]]), markers, counts, ("4100 frames", f))
    det.close()


def test_crop_rings_of_more_than_18432_crops(oa):
    """9 frames of 1920 x 1080 with 2205 squares each on a dense context: more crop ROIs than the 9 * 32 waves of
    ring_quads_kernel<true> take in one trip of 64 each"""
    distinct, index = R.dense_scene()
    W, Hh, n = R.DENSE_W, R.DENSE_H, len(index)
    tpls, cam = H.oracle_templates(), H.oracle_camera(W, Hh)
    refs = []
    for g in distinct:
        ref = OracleFrame.__new__(OracleFrame)
        ref.markers, ref.cands, _ = H.oracle_registration(R.bgr(g), tpls, cam, max_markers=20000, max_cands=200000)
        ref.w, ref.h, ref.grey, ref.cand_arr = W, Hh, g, None
        ref.binary = H.oracle_binarise(g)
        ref.masks = H.neighbour_masks(ref.binary)
        ref.quads = None   # (debug_frame_quads holds OCVAR_MAX_QUADS quads; the candidates carry every square)
        refs.append(ref)
    det = oa.Detector(W, Hh, max_batch=n, max_quads=R.DENSE_QUADS, max_markers=R.DENSE_MARKERS)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    markers, counts = det.detect_host(np.stack([R.bgr(distinct[k]) for k in index]))
    by_pos = {f: refs[index[f]] for f in range(n)}
    verdicts, rois, crop_verdicts = check_rings(det, n, W, Hh, "dense", by_pos, crop_planes_of={0})
    assert len(rois) > R.DENSE_MIN_ROIS and verdicts.all()
    holed = int((crop_verdicts == 0).sum())
    assert 6 * holed >= len(rois) and 2 * holed <= len(rois), (holed, len(rois))
    for f in (0, 1):   # (one position of each distinct frame: planes; every position: end results)
        check_planes(det, f, by_pos[f], ("dense", f))
    for f in range(n):
        check_candidates(det, f, by_pos[f], ("dense", f))
        check_markers(f, by_pos[f], markers, counts, ("dense", f))
    det.close()


def test_flags_of_a_small_batch_are_cleared_not_stale(oa):
    """130 crops in 9 frames, then the same frames cut to 8 -- no ring kernel runs: api.hip and order.hip clear the flags --, then
    9 frames with one crop"""
    big, cut, one = R.stale_sequence()
    W, Hh = big.shape[2], big.shape[1]
    det, _, _ = make_detector(oa, size(W, Hh), None, 9)
    det.detect_host(big.copy())
    verdicts, rois, crop_verdicts = check_rings(det, 9, W, Hh, "130 crops")
    assert verdicts.all() and len(rois) == 130 and 0 < crop_verdicts.sum() < 130
    det.detect_host(cut.copy())
    ff, cf = det.debug_rings(False), det.debug_rings(True)
    assert len(ff) == 8 and len(cf) == len(det.debug_crops()) == 130 and not ff.any() and not cf.any(), (ff.tolist(), cf.tolist())
    det.detect_host(one.copy())
    verdicts, rois, crop_verdicts = check_rings(det, 9, W, Hh, "1 crop")
    assert verdicts.all() and len(rois) == 1 and len(det.debug_rings(True)) == 1 and crop_verdicts.tolist() == [1]
    det.close()

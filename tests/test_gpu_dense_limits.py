"""GPU tests of dense contexts at their limits, against the oracle: frames with exactly max_quads squares, one more, one fewer
(every change of order_chunk, of the sort's block size and of decode_slices, partial last chunks), exactly max_markers
markers and one more (stateless and tracked, detect_host(prev=) and enqueue_tracked), mixed batches that check the per-frame
strides, adversarial `prev` arrays for the tracking replay's corner grid, crop pools at density, and the top of
libopencv-ar.so's retry ladder.  The frame builders are in tests/dense_synth.py (their exact counts: test_dense_cpu.py)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dense_synth as D
import helpers as H
from frame_kit import oa  # noqa: F401
from hostbuild import host_driver

pytestmark = pytest.mark.gpu

FLAG_QUADS, FLAG_CROPS, FLAG_TILES, FLAG_MARKERS = 4, 16, 32, 128
QS = [1, 63, 64, 65, 255, 256, 2047, 2048, 2049, 4097, 16384]
MS = [1, 7, 64, 65]          # (4096: test_marker_cap_4096_through_tracked_markers)
POOL = 16


def pmap(fn, items):
    with ThreadPoolExecutor(POOL) as ex:
        return list(ex.map(fn, items))


def check_records(got, count, ref, what):
    """count equals the oracle's; every field of every record byte for byte, the pose within the 1e-4 bar"""
    assert count == len(ref), (what, count, len(ref))
    for k, r in enumerate(ref):
        m = got[k]
        want = np.frombuffer(bytes(r), m.dtype)[0]
        for name in ("templateId", "markerId", "score", "square", "aspectRatio"):
            assert np.asarray(m[name]).tobytes() == np.asarray(want[name]).tobytes(), (what, k, name, m[name], want[name])
        g = np.asarray(want["glMatrix"])
        assert np.abs(m["glMatrix"] - g).max() <= 1e-4 * max(1.0, np.abs(g).max()), (what, k, "glMatrix")


def check_candidates(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a.markerId, a.templateId, a.orient, a.bit) == (b.markerId, b.templateId, b.orient, b.bit), (what, k)
        assert list(a.square) == list(b.square) and list(a.patPoint) == list(b.patPoint), (what, k)


def bgr(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def dense(oa, w, h, q, m, tpls, cam, batch=1):
    det = oa.Detector(w, h, max_batch=batch, max_quads=q, max_markers=m)
    assert det.max_quads == q and det.max_markers == m
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    return det


def flags(oa, det):
    return oa.hip_lib().ocvar_hip_capacity_flags(det._ctx)


def marker_rows(oa, ms):
    rows = np.zeros(len(ms), oa.MARKER_DTYPE)
    for k, m in enumerate(ms):
        rows[k] = np.frombuffer(bytes(m), oa.MARKER_DTYPE)[0]
    return rows


# ---- the square cap ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib3():
    names = D.library(3)
    return names, H.oracle_templates(names)


@pytest.fixture(scope="module")
def square_frames(lib3):
    """n -> (grey frame with exactly n oracle squares, its oracle squares, markers, candidates) for n in Q - 1, Q, Q + 1"""
    ns = sorted({n for q in QS for n in (q - 1, q, q + 1)})
    tpls = lib3[1]

    def one(n):
        g = D.squares_frame(n)
        h, w = g.shape
        m, c, _ = H.oracle_registration(bgr(g), tpls, H.oracle_camera(w, h), max_markers=20000, max_cands=200000)
        return n, (g, D.oracle_squares(g), m, c)
    return dict(pmap(one, ns))


@pytest.mark.parametrize("q", QS)
def test_square_cap(oa, lib3, square_frames, q):
    """Q - 1 and Q squares: the oracle's find_squares sequence, markers and candidates, no flag; Q + 1: OcvarError, flag 4,
    and nothing handed out"""
    tpls = lib3[1]
    for n in (q - 1, q, q + 1):
        g, ref_sq, ref_m, ref_c = square_frames[n]
        h, w = g.shape
        det = dense(oa, w, h, q, 64, tpls, H.oracle_camera(w, h))
        det.set_input_format("gray")
        if n <= q:
            quads, got_n = det.find_squares(g)
            assert got_n == n and np.array_equal(quads, ref_sq), (q, n)
            markers, counts = det.detect_host(np.ascontiguousarray(g[None]))
            assert flags(oa, det) == 0
            check_records(markers[0], counts[0], ref_m, (q, n))
            check_candidates(det.debug_candidates(0), ref_c, (q, n))
        else:
            with pytest.raises(oa.OcvarError):
                det.find_squares(g)
            assert flags(oa, det) & FLAG_QUADS, (q, n)
            with pytest.raises(oa.OcvarError):
                det.detect_host(np.ascontiguousarray(g[None]))
            assert flags(oa, det) & FLAG_QUADS, (q, n)
        det.close()


@pytest.mark.parametrize("q", [64, 2049, 16384])
def test_square_cap_mixed_batch(oa, lib3, q):
    """frames of Q, 0, 1, Q - 1 squares at several batch positions (the last one included): frame f's squares, records and
    tracking arrays stay at f * Q / f * M"""
    tpls = lib3[1]
    w, h = D.frame_size_for(q)
    counts_in = [q, 0, 1, q - 1, q, 1, 0, q]
    frames = {n: D.squares_frame(n, w, h) for n in set(counts_in)}
    cam = H.oracle_camera(w, h)
    refs = dict(pmap(lambda n: (n, H.oracle_registration(bgr(frames[n]), tpls, cam, max_markers=20000, max_cands=200000)[:2]),
                     sorted(frames)))
    # every square of frame f carried in as a previous marker of frame f (at most M): the tracking arrays per frame
    M = 64
    prevs = []
    for f, n in enumerate(counts_in):
        sq = D.oracle_squares(frames[n])[f % 3::3][:M - 16]   # (room for the markers the untracked squares decode to)
        prev = (H.Marker * len(sq))()
        for i, s in enumerate(sq):
            prev[i].square[:] = [float(v) for v in s.reshape(-1)]
            prev[i].templateId, prev[i].markerId, prev[i].score, prev[i].aspectRatio = f, i, 1.0, 1.0
        prevs.append(list(prev))
    ref_t = pmap(lambda f: H.oracle_registration(bgr(frames[counts_in[f]]), tpls, cam, prev=prevs[f], max_markers=20000,
                                                 max_cands=200000)[:2], range(len(counts_in)))
    det = dense(oa, w, h, q, M, tpls, cam, batch=len(counts_in))
    det.set_input_format("gray")
    batch = np.ascontiguousarray(np.stack([frames[n] for n in counts_in]))
    markers, counts = det.detect_host(batch)
    assert flags(oa, det) == 0
    for f, n in enumerate(counts_in):
        check_records(markers[f], counts[f], refs[n][0], ("stateless", q, f))
        check_candidates(det.debug_candidates(f), refs[n][1], ("stateless", q, f))
    markers, counts = det.detect_host(batch, prev=[list(marker_rows(oa, p)) for p in prevs])
    assert flags(oa, det) == 0
    for f in range(len(counts_in)):
        check_records(markers[f], counts[f], ref_t[f][0], ("tracked", q, f))
        check_candidates(det.debug_candidates(f), ref_t[f][1], ("tracked", q, f))
    # one frame past Q at the last position: the batch fails with flag 4
    bad = batch.copy()
    bad[-1] = D.squares_frame(q + 1, w, h)
    with pytest.raises(oa.OcvarError):
        det.detect_host(bad)
    assert flags(oa, det) & FLAG_QUADS


# ---- the marker cap ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib66():
    names = D.library(66, seed=11)
    return names, H.oracle_templates(names)


@pytest.fixture(scope="module")
def marker_cases(lib66):
    """target -> stateless (frame, oracle markers, candidates) with exactly `target` markers, for every M - 1, M, M + 1"""
    names, tpls = lib66
    cam = H.oracle_camera(1920, 1080)
    ks = sorted({k for m in MS for k in (m - 1, m, m + 1)})

    def one(k):
        f = D.marker_frame(k, names)
        m, c, _ = H.oracle_registration(f, tpls, cam, max_markers=20000, max_cands=200000)
        assert len(m) == k, (k, len(m))
        return k, (f, m, c)
    return dict(pmap(one, ks))


@pytest.fixture(scope="module")
def tracked_cases(lib66, marker_cases):
    """(M, target) -> (frame, prev, oracle markers): prev (at most M markers, from a stateless result) carried in so that the
    tracked plus the new markers total exactly target, for target M and M + 1"""
    names, tpls = lib66
    cam = H.oracle_camera(1920, 1080)

    def one(mt):
        M, target = mt
        for k in (target, target - 1, target + 1):
            if k not in marker_cases or k < 1:
                continue
            f, stateless, _ = marker_cases[k]
            for p in range(min(k, M), 0, -1):
                ref, _, _ = H.oracle_registration(f, tpls, cam, prev=stateless[:p], max_markers=20000, max_cands=1)
                if len(ref) == target:
                    return mt, (f, list(stateless[:p]), ref)
        raise AssertionError(f"no tracked case with {target} markers")
    return dict(pmap(one, [(m, t) for m in MS for t in (m, m + 1)]))


@pytest.mark.parametrize("M", MS)
def test_marker_cap_stateless(oa, lib66, marker_cases, M):
    tpls = lib66[1]
    cam = H.oracle_camera(1920, 1080)
    det = dense(oa, 1920, 1080, 1024, M, tpls, cam)
    for k in (M - 1, M, M + 1):
        f, ref, ref_c = marker_cases[k]
        if k <= M:
            markers, counts = det.detect_host(np.ascontiguousarray(f[None]))
            assert flags(oa, det) == 0
            check_records(markers[0], counts[0], ref, ("stateless", M, k))
            check_candidates(det.debug_candidates(0), ref_c, ("stateless", M, k))
        else:
            with pytest.raises(oa.OcvarError):
                det.detect_host(np.ascontiguousarray(f[None]))
            assert flags(oa, det) == FLAG_MARKERS, (M, k)


@pytest.mark.parametrize("M", MS)
def test_marker_cap_tracked(oa, lib66, tracked_cases, M):
    """detect_host(prev=) and enqueue_tracked (prev in device memory): M markers equal the oracle, M + 1 raise flag 128"""
    import torch
    tpls = lib66[1]
    cam = H.oracle_camera(1920, 1080)
    det = dense(oa, 1920, 1080, 1024, M, tpls, cam)
    dev = dense(oa, 1920, 1080, 1024, M, tpls, cam)
    for target in (M, M + 1):
        f, prev, ref = tracked_cases[(M, target)]
        assert len(prev) <= M
        rows = marker_rows(oa, prev)
        pm = np.zeros((1, M), oa.MARKER_DTYPE)
        pm[0, :len(prev)] = rows
        d_prev = torch.from_numpy(pm.view(np.uint8)).cuda()
        d_cnt = torch.tensor([len(prev)], dtype=torch.int32, device="cuda")
        d_frame = torch.from_numpy(np.ascontiguousarray(f[None])).cuda()
        torch.cuda.synchronize()
        if target <= M:
            markers, counts = det.detect_host(np.ascontiguousarray(f[None]), prev=[list(rows)])
            assert flags(oa, det) == 0
            check_records(markers[0], counts[0], ref, ("detect_host", M, target))
            dev.enqueue_tracked(d_frame.data_ptr(), 1920, 1080, 1, d_prev.data_ptr(), d_cnt.data_ptr())
            m2, c2 = dev.collect()
            assert flags(oa, dev) == 0
            check_records(m2[0], c2[0], ref, ("enqueue_tracked", M, target))
        else:
            with pytest.raises(oa.OcvarError):
                det.detect_host(np.ascontiguousarray(f[None]), prev=[list(rows)])
            assert flags(oa, det) == FLAG_MARKERS, (M, target)
            dev.enqueue_tracked(d_frame.data_ptr(), 1920, 1080, 1, d_prev.data_ptr(), d_cnt.data_ptr())
            with pytest.raises(oa.OcvarError):
                dev.collect()
            assert flags(oa, dev) == FLAG_MARKERS, (M, target)


@pytest.fixture(scope="module")
def cap4096(lib3):
    """3840 x 2160 frames: one decodable marker (a strip at the top) and solid squares; every solid square carried in as a
    previous marker (up to 4096 of them) -- the tracked ones plus the decoded one total 4096 and 4097.  The library cannot
    exceed 4096 templates: M + 1 is reached through tracked markers."""
    names, tpls = lib3
    cam = H.oracle_camera(3840, 2160)
    strip = D.marker_strip(1, names)
    strip_sq = D.strip_squares(strip, 3840, 2160)
    out = {}
    for target in (4096, 4097):
        g = D.squares_frame(strip_sq + target - 1, 3840, 2160, marker_strip=strip)
        sq = D.oracle_squares(g)
        solid = [s for s in sq if s[:, 1].min() >= strip.shape[0]]
        prev = (H.Marker * len(solid))()
        for i, s in enumerate(solid):
            prev[i].square[:] = [float(v) for v in s.reshape(-1)]
            prev[i].templateId, prev[i].markerId, prev[i].score, prev[i].aspectRatio = i % 3, i, 1.0, 1.0
        assert len(solid) == target - 1 <= 4096
        ref, _, _ = H.oracle_registration(bgr(g), tpls, cam, prev=list(prev), max_markers=20000, max_cands=1)
        assert len(ref) == target, (target, len(ref))
        out[target] = (g, list(prev), ref)
    return out


def test_marker_cap_4096_through_tracked_markers(oa, lib3, cap4096):
    import torch
    tpls = lib3[1]
    cam = H.oracle_camera(3840, 2160)
    det = dense(oa, 3840, 2160, 16384, 4096, tpls, cam)
    det.set_input_format("gray")
    for target in (4096, 4097):
        g, prev, ref = cap4096[target]
        rows = marker_rows(oa, prev)
        pm = np.zeros((1, 4096), oa.MARKER_DTYPE)
        pm[0, :len(prev)] = rows
        d_prev = torch.from_numpy(pm.view(np.uint8)).cuda()
        d_cnt = torch.tensor([len(prev)], dtype=torch.int32, device="cuda")
        d_frame = torch.from_numpy(np.ascontiguousarray(g[None])).cuda()
        torch.cuda.synchronize()
        if target == 4096:
            markers, counts = det.detect_host(np.ascontiguousarray(g[None]), prev=[list(rows)])
            assert flags(oa, det) == 0
            check_records(markers[0], counts[0], ref, ("detect_host", target))
            det.enqueue_tracked(d_frame.data_ptr(), 3840, 2160, 1, d_prev.data_ptr(), d_cnt.data_ptr())
            m2, c2 = det.collect()
            check_records(m2[0], c2[0], ref, ("enqueue_tracked", target))
        else:
            with pytest.raises(oa.OcvarError):
                det.detect_host(np.ascontiguousarray(g[None]), prev=[list(rows)])
            assert flags(oa, det) == FLAG_MARKERS
            det.enqueue_tracked(d_frame.data_ptr(), 3840, 2160, 1, d_prev.data_ptr(), d_cnt.data_ptr())
            with pytest.raises(oa.OcvarError):
                det.collect()
            assert flags(oa, det) == FLAG_MARKERS


# ---- adversarial prev ------------------------------------------------------------------------------------------------------

def mk(square, tid=0, mid=0):
    m = H.Marker()
    m.square[:] = [float(v) for v in np.asarray(square, np.float64).reshape(-1)]
    m.templateId, m.markerId, m.score, m.aspectRatio = tid, TRACKED_ID + mid, 1.0, 1.0   # (ids no decoded marker has)
    return m


TRACKED_ID = 100000


def n_tracked(ref):
    return sum(r.markerId >= TRACKED_ID for r in ref)


def adversarial_prevs(sq, w, h, rng):
    """name -> list of markers built from a frame's oracle squares sq [n, 4, 2]"""
    sq = sq.astype(np.float64)
    pick = sq[rng.choice(len(sq), min(len(sq), 48), replace=False)]
    out = {}
    for d in (19.9, 20.0, 20.1):
        for name, off in (("x", (d, 0)), ("y", (0, d)), ("-x", (-d, 0)), ("-y", (0, -d))):
            out[f"shift{name}{d}"] = [mk(s + np.array(off), i % 3, i) for i, s in enumerate(pick)]
            c0 = [s.copy() for s in pick]
            for s in c0:
                s[0] += off
            out[f"corner0{name}{d}"] = [mk(s, i % 3, i) for i, s in enumerate(c0)]
    # corner 0 moved across the nearest 32 px cell border in x and y (less than 20 px away from where it was)
    strad = []
    for i, s in enumerate(pick):
        t = s.copy()
        for a in (0, 1):
            b = np.round(s[0, a] / 32) * 32
            t[:, a] += (b - 0.25 if s[0, a] >= b else b + 0.25) - s[0, a]
        strad.append(mk(t, i % 3, i))
    out["straddle"] = strad
    # corners off the frame: negative, past W / H, past 2^15 (some of them within 20 px of a square near the border)
    off = [mk(s - np.array([s[:, 0].min() + 10, 0]), 0, i) for i, s in enumerate(pick[:8])]
    off += [mk(s - np.array([0, s[:, 1].min() + 10]), 1, i) for i, s in enumerate(pick[:8])]
    off += [mk(s + np.array([w - s[:, 0].max() + 5, 0]), 2, i) for i, s in enumerate(pick[:8])]
    off += [mk(s + np.array([0, h - s[:, 1].max() + 5]), 0, i) for i, s in enumerate(pick[:8])]
    off += [mk(s + np.array([40000, 0]), 1, i) for i, s in enumerate(pick[:4])]
    off += [mk(s + np.array([0, 1e9]), 2, i) for i, s in enumerate(pick[:4])]
    off += [mk(np.full((4, 2), -70000.0), 0, 99)]
    # the squares nearest the left and top borders, moved 10 px past them: negative corners within 20 px of a square
    for a in (0, 1):
        s = sq[np.argmin(sq[:, :, a].min(axis=1))]
        t = s.copy()
        t[:, a] -= s[:, a].min() + 10
        assert s[:, a].min() + 10 < 20
        off.append(mk(t, a, 200 + a))
    out["offframe"] = off + [mk(s, i % 3, i) for i, s in enumerate(pick[:16])]
    bad = []
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        for k in range(8):
            t = pick[k % len(pick)].copy()
            t.reshape(-1)[(k + i) % 8] = v
            bad.append(mk(t, i, k))
            bad.append(mk(np.full((4, 2), v), i, 100 + k))
    out["nonfinite"] = bad + [mk(s, i % 3, i) for i, s in enumerate(pick[:16])]
    out["repeated"] = [mk(pick[0], 1, 7)] * 300 + [mk(s, i % 3, i) for i, s in enumerate(pick[1:20])]
    jit = rng.uniform(-6, 6, (300, 4, 2))
    out["one_cell"] = [mk(pick[0] + jit[i] * (i > 0), i % 3, i) for i in range(300)]
    out["cyclic"] = [mk(np.roll(s, -r, axis=0), r % 3, i) for i, s in enumerate(pick[:24]) for r in range(4)]
    out["reversed"] = [mk(s[::-1], i % 3, i) for i, s in enumerate(pick[:24])]
    return out


@pytest.fixture(scope="module")
def adversarial(lib3):
    """(frame name, prev name) -> (grey frame, prev, oracle markers, candidates)"""
    tpls = lib3[1]
    rng = np.random.default_rng(5)
    frames = {}
    for w, h in ((3839, 2157), (1001, 999)):
        frames[f"{w}x{h}"] = D.squares_frame(len(D.square_slots(w, h, margin=4)), w, h, margin=4)
    frames["1001x999_small"] = D.squares_frame(200, 1001, 999, margin=4)
    jobs = []
    for fn, g in frames.items():
        h, w = g.shape
        for pn, prev in adversarial_prevs(D.oracle_squares(g), w, h, rng).items():
            jobs.append((fn, pn, prev))

    def one(job):
        fn, pn, prev = job
        g = frames[fn]
        h, w = g.shape
        m, c, _ = H.oracle_registration(bgr(g), tpls, H.oracle_camera(w, h), prev=prev, max_markers=20000, max_cands=200000)
        return (fn, pn), (g, prev, m, c)
    return dict(pmap(one, jobs))


def test_adversarial_prev(oa, lib3, adversarial):
    """the replay's 32 px corner grid against the reference's literal loop, with prev arrays a caller may legally pass"""
    tpls = lib3[1]
    dets, small = {}, {}
    tracked_any = set()
    for (fn, pn), (g, prev, ref, ref_c) in sorted(adversarial.items(), key=lambda kv: kv[0]):
        h, w = g.shape
        if fn not in dets:
            dets[fn] = dense(oa, w, h, 16384, 4096, tpls, H.oracle_camera(w, h))
            dets[fn].set_input_format("gray")
        det = dets[fn]
        rows = marker_rows(oa, prev)
        markers, counts = det.detect_host(np.ascontiguousarray(g[None]), prev=[list(rows)])
        assert flags(oa, det) == 0
        check_records(markers[0], counts[0], ref, (fn, pn))
        check_candidates(det.debug_candidates(0), ref_c, (fn, pn))
        if n_tracked(ref):
            tracked_any.add(pn)
        if fn == "1001x999_small" and len(prev) <= 64 and len(ref) <= 64:
            # a default context (the literal tracking loop) gives the same bytes
            if fn not in small:
                small[fn] = oa.Detector(w, h, max_batch=1)
                small[fn].set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in tpls])
                small[fn].set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(w, h))))
                small[fn].set_input_format("gray")
            m2, c2 = small[fn].detect_host(np.ascontiguousarray(g[None]), prev=[list(rows)])
            assert c2[0] == counts[0]
            assert m2[0, :c2[0]].tobytes() == markers[0, :counts[0]].tobytes(), (fn, pn)
    # the cases reach the match window's edges from both sides
    assert {"shiftx19.9", "corner0x19.9", "straddle", "offframe", "cyclic", "one_cell", "repeated"} <= tracked_any
    # (exactly 20 px from the square and from its neighbour 40 px on: no match; 20.1 px is 19.9 px from the neighbour)
    for d in ("20.0",):
        assert not any(n_tracked(adversarial[(fn, f"shift{a}{d}")][2]) for fn in ("3839x2157", "1001x999") for a in ("x", "y"))


# ---- crop pools at density -----------------------------------------------------------------------------------------------

def test_crop_pools_at_density(oa, lib3, square_frames):
    """the Q = 16384 frame and a frame of concentric squares whose crops overlap: the oracle's answer, or OCVAR_E_CAPACITY
    with flag 16 / 32 -- never a different answer.  The 16384 non-overlapping squares must fit the pools."""
    tpls = lib3[1]
    conc = D.concentric_frame(3840, 2160)
    ref_conc = H.oracle_registration(bgr(conc), tpls, H.oracle_camera(3840, 2160), max_markers=20000, max_cands=400000)[:2]
    assert len(D.oracle_squares(conc)) <= 16384
    grid = square_frames[16384]
    for name, g, q, (ref, ref_c) in (("grid16384", grid[0], 16384, grid[2:]), ("concentric", conc, 16384, ref_conc)):
        h, w = g.shape
        cam = H.oracle_camera(w, h)
        det = dense(oa, w, h, q, 4096, tpls, cam)
        det.set_input_format("gray")
        try:
            markers, counts = det.detect_host(np.ascontiguousarray(g[None]))
        except oa.OcvarError:
            fl = flags(oa, det)
            assert name != "grid16384", (name, fl)   # (non-overlapping squares: the header's promise)
            assert fl & (FLAG_CROPS | FLAG_TILES) and not fl & ~(FLAG_CROPS | FLAG_TILES), (name, fl)
            continue
        assert flags(oa, det) == 0
        check_records(markers[0], counts[0], ref, name)
        check_candidates(det.debug_candidates(0), ref_c, name)


# ---- the top of libopencv-ar.so's retry ladder (each case in a fresh process) -----------------------------------------------

FIND_SQUARES_CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import opencv_ar_amd as oa
from test_gpu_boundary import CvSeq, ipl, seq_points
oa.hip_lib()
g = np.load(sys.argv[2])
host = C.CDLL(oa.HOST_LIB)
host.cvarFindSquares.restype = C.POINTER(CvSeq)
host.cvarFindSquares.argtypes = [C.c_void_p, C.c_void_p]
img_arr = np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
img = ipl(img_arr)
seq = host.cvarFindSquares(C.byref(img), None)
np.save(sys.argv[3], seq_points(seq) if seq.contents.total else np.zeros((0, 4, 2), np.int32))
"""


def test_host_ladder_find_squares_top(oa, square_frames, tmp_path):
    """cvarFindSquares climbs 256 -> .. -> 16384: exactly 16384 squares give the oracle's whole sequence; 16385 give an empty
    sequence and a report on stderr, not a truncated list"""
    script = tmp_path / "child.py"
    script.write_text(FIND_SQUARES_CHILD)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([H.ROOT, os.path.join(H.ROOT, "tests")]))
    for n in (16384, 16385):
        g, ref, _, _ = square_frames[n]
        inp, out = tmp_path / f"g{n}.npy", tmp_path / f"q{n}.npy"
        np.save(inp, g)
        r = subprocess.run([sys.executable, str(script), H.ROOT, str(inp), str(out)], capture_output=True, text=True, timeout=300,
                           env=env)
        assert r.returncode == 0, r.stderr
        got = np.load(out)
        if n == 16384:
            assert np.array_equal(got, ref)
        else:
            assert len(got) == 0
            assert "cvarFindSquares failed" in r.stderr


def run_tracking_driver(oa, tmp_path, w, h, tpls, cam, initial, frames, tag):
    exe = host_driver("tracking_driver")
    inp, out = tmp_path / f"in_{tag}.bin", tmp_path / f"out_{tag}.bin"
    inp.write_bytes(np.array([w, h, len(tpls), len(frames), len(initial)], np.int32).tobytes() + bytes(tpls) + bytes(cam) +
                    b"".join(bytes(m) for m in initial) + b"".join(f.tobytes() for f in frames))
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw, off, steps = out.read_bytes(), 0, []
    for _ in frames:
        count, n_out = np.frombuffer(raw[off:off + 8], np.int32)
        off += 8
        steps.append((int(count), np.frombuffer(raw[off:off + n_out * oa.MARKER_DTYPE.itemsize], oa.MARKER_DTYPE)))
        off += n_out * oa.MARKER_DTYPE.itemsize
    return steps, r.stderr


def test_host_ladder_registration_top(oa, lib3, cap4096, tmp_path):
    """cvarArMultRegistration: 4096 markers equal the oracle (a context with the top marker stride); 4097 markers out of the
    frame, or more than 4096 carried in, return 0 with an empty vector"""
    tpls = lib3[1]
    cam = H.oracle_camera(3840, 2160)
    for target in (4096, 4097):
        g, prev, ref = cap4096[target]
        steps, err = run_tracking_driver(oa, tmp_path, 3840, 2160, tpls, cam, prev, [bgr(g)], f"t{target}")
        count, got = steps[0]
        if target == 4096:
            check_records(got, count, ref, ("ladder", target))
        else:
            assert count == 0 and len(got) == 0, (count, len(got))
            assert "detection failed" in err
    g, prev, _ = cap4096[4097]
    steps, err = run_tracking_driver(oa, tmp_path, 3840, 2160, tpls, cam, prev + prev[:2], [bgr(g)], "carried")
    assert steps[0][0] == 0 and len(steps[0][1]) == 0

"""Parity under the load the project's numbers are measured at: the benchmark's schedule (bench.py: 5 contexts on their own
streams sharing a gate of 2, ~1638-frame launches, ragged first launches) and the pipe at its defaults (ocvar_hip_pipe_*: 2048-
frame chunks over 4 contexts, gate 2), every output compared with the oracle.

Round 3's worst bug corrupted mask words only from the 16th frame of a batch on and only while the memory system was busy
(the buffer stores' scalar offset field); small batches never show such a fault.  Here the batches are thousands of
frames.  U distinct seeded frames (textured backgrounds, corner jitter, occlusion, noise / contrast / colour cast / blur, the
shipped templates and the 5x5..8x8 grids) are tiled on the device, so every batch position sees several different frames and
the oracle runs U times."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers as H
from frame_kit import oa  # noqa: F401
from test_gpu_parity import OracleFrame, check_candidates, check_markers, check_planes

pytestmark = pytest.mark.gpu

NAMES = H.TEMPLATE_ORDER + H.BIG_TEMPLATES
NS, GATE = 5, 2          # bench.py defaults: --streams 5 --gate 2
SHIFT = 7                # frame f of context i is distinct frame (f + SHIFT * i) % U


def distinct_frames(w, h, n, seed):
    """n seeded frames with the variety of tools/fuzz_parity.py: marker grid, sizes, rotations, jitter, occlusion, background,
    a random subset of NAMES planted, then one of the post-processing modes"""
    rng = np.random.default_rng(seed)
    specs = []
    for u in range(n):
        side_min = int(rng.integers(60, 130))
        cell = max(side_min + 60, 140)
        cfg = H.synth_config(3, width=w, height=h, grid_x=max(1, min(8, w // (cell + 40))), grid_y=max(1, min(8, h // (cell + 40))),
                             side_min=side_min, side_max=side_min + int(rng.integers(0, 60)), rot_mode=int(rng.integers(0, 3)),
                             corner_jitter_pct=int(rng.integers(0, 12)), occlude_pct=int(rng.choice([0, 0, 20, 50])),
                             textured=int(rng.integers(0, 2)))
        names = [NAMES[i] for i in sorted(rng.choice(len(NAMES), size=int(rng.integers(1, 5)), replace=False))]
        specs.append((cfg, int(rng.integers(0, 1 << 20)), names, int(rng.integers(0, 5)), int(rng.integers(0, 1 << 30))))

    def make(spec):
        cfg, idx, names, mode, s2 = spec
        r = np.random.default_rng(s2)
        img = H.synth_frame(cfg, idx, names)[0].astype(np.int32)
        if mode == 1:      # sensor noise, per channel
            img += r.integers(-9, 10, img.shape)
        elif mode == 2:    # low contrast + offset
            img = img * int(r.integers(30, 90)) // 100 + int(r.integers(0, 80))
        elif mode == 3:    # colour cast
            img = img * np.array([r.integers(60, 101), r.integers(60, 101), r.integers(60, 101)]) // 100
        elif mode == 4:    # 3-tap blur along x
            img = (img + np.roll(img, 1, 1) + np.roll(img, -1, 1)) // 3
        return np.clip(img, 0, 255).astype(np.uint8)

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        return np.stack(list(ex.map(make, specs)))


def oracle_all(base, tpls, cam, prev=None, planes=True):
    with ThreadPoolExecutor(min(32, os.cpu_count() or 1)) as ex:   # (the oracle is C; ctypes releases the GIL)
        return list(ex.map(lambda u: OracleFrame(base[u], tpls, cam, prev=None if prev is None else prev[u], planes=planes),
                           range(len(base))))


class Scene:
    """U distinct frames, their oracle results, and a device array T with T[j] = base[j % U] of n_dev frames"""

    def __init__(self, w, h, U, n_dev, seed):
        import torch
        self.w, self.h, self.U = w, h, U
        self.tpls, self.cam = H.oracle_templates(NAMES), H.oracle_camera(w, h)
        self.base = distinct_frames(w, h, U, seed)
        self.refs = oracle_all(self.base, self.tpls, self.cam)
        self.d_base = torch.from_numpy(self.base).cuda()
        self.d = self.d_base[torch.arange(n_dev, device="cuda") % U].contiguous()
        torch.cuda.synchronize()
        self.fb = w * h * 3

    def ptr(self, j):
        return self.d.data_ptr() + j * self.fb

    def templates(self, oa):
        return [oa.Template.from_buffer_copy(bytes(t)) for t in self.tpls]

    def camera(self, oa):
        return oa.Camera.from_buffer_copy(bytes(self.cam))

    def close(self):
        import torch
        del self.d, self.d_base
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("w,h,launch,U", [(1920, 1080, 1638, 64), (3840, 2160, 410, 16)], ids=["1080p-1638", "2160p-410"])
def test_parity_at_the_benchmark_geometry(oa, w, h, launch, U):
    """bench.py's schedule built from Detectors: 5 contexts on their own streams sharing Gate(2), context i's first launch
    (i + 1) * launch / 5 frames, then a full launch enqueued right behind the collect of the first while the other contexts run,
    result limit 8 and collect(8) as bench.py.  Every frame of every launch: count and marker records against the oracle.
    Every frame of each context's last launch (the workspace holds the last batch): pre-dedupe candidates, i.e. the crop pass
    under load.  A fixed sample of >= 256 positions of the last launches, the last 64 of each among them: grey plane, binary
    image and every bit of the mask plane."""
    first = [max(1, ((i + 1) * launch) // NS) for i in range(NS)]
    sc = Scene(w, h, U, max(first) + launch + SHIFT * (NS - 1), seed=1000 + w)
    try:
        gate = oa.Gate(GATE)
        dets = []
        for i in range(NS):
            det = oa.Detector(w, h, max_batch=launch)
            det.set_templates(sc.templates(oa))
            det.set_camera(sc.camera(oa))
            det.set_gate(gate)
            det.set_result_limit(8)
            dets.append(det)
        starts = [[0, first[i]] for i in range(NS)]          # sequence index of each launch's first frame, per context
        sizes = [[first[i], launch] for i in range(NS)]
        for i in range(NS):
            dets[i].enqueue_device(sc.ptr(SHIFT * i), w, h, first[i])
        got = [[None, None] for _ in range(NS)]
        for i in range(NS):
            got[i][0] = dets[i].collect(8)
            dets[i].enqueue_device(sc.ptr(SHIFT * i + first[i]), w, h, launch)
        for i in range(NS):
            got[i][1] = dets[i].collect(8)
        frames = 0
        for i in range(NS):
            for L in range(2):
                m, c = got[i][L]
                assert len(c) == sizes[i][L]
                for p in range(sizes[i][L]):
                    u = (starts[i][L] + p + SHIFT * i) % U
                    check_markers(p, sc.refs[u], m, c, where=f"context {i} launch {L} position {p} frame {u}")
                frames += len(c)
        n_markers = sum(len(sc.refs[(starts[i][L] + p + SHIFT * i) % U].markers) for i in range(NS) for L in range(2)
                        for p in range(sizes[i][L]))
        assert n_markers >= frames   # (the scene plants markers: the comparison is not of empty results)
        rng = np.random.default_rng(7)
        sampled = 0
        for i in range(NS):
            last = starts[i][1]
            for p in range(launch):
                check_candidates(dets[i], p, sc.refs[(last + p + SHIFT * i) % U], where=f"context {i} launch 1 position {p}")
            spread = rng.choice(launch - 64, size=min(launch - 64, 40), replace=False)
            for p in sorted(set(spread.tolist()) | set(range(launch - 64, launch))):
                check_planes(dets[i], p, sc.refs[(last + p + SHIFT * i) % U], where=f"context {i} launch 1 position {p}")
                sampled += 1
        assert sampled >= 256
        del dets, det, gate
    finally:
        sc.close()


def test_benchmark_outputs_against_the_oracle(tmp_path):
    """bench.py's own timed outputs (a child process: --steps 2 --warmup 1 --dump-outputs) through tools/check_bench_dump.py:
    every frame of the default 8192-frame batch, count and records against the oracle.  (Before the pipe tests below: their
    module-scoped scene and contexts hold device memory the child's 8192-frame batch needs.)"""
    import gc
    import subprocess
    import sys
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-latency", "--dump-outputs", out], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import check_bench_dump
    n, n_records = check_bench_dump.check_dump(out, config=3, unique=256)
    assert n == 8192 and n_records >= n


@pytest.fixture(scope="module")
def hd(oa):
    """1080p scene of 64 distinct frames tiled to PIPE_N on the device; the pipe at its defaults"""
    sc = Scene(1920, 1080, 64, PIPE_N, seed=77)
    pipe = oa.Pipe(sc.w, sc.h)
    assert pipe.chunk_frames == 2048
    pipe.set_templates(sc.templates(oa))
    pipe.set_camera(sc.camera(oa))
    yield sc, pipe
    pipe.close()
    sc.close()


PIPE_N = 512 + 1024 + 1536 + 2048 + 2048 + 700   # 4 ragged chunks (k + 1) / 4 of 2048, one full chunk, a partial one


def check_rows(sc, m, c, j0, where):
    for p in range(len(c)):
        check_markers(p, sc.refs[(j0 + p) % sc.U], m, c, where=f"{where} frame {j0 + p}")


def test_pipe_detect_device_at_its_defaults(hd):
    """ocvar_hip_pipe_detect_device over PIPE_N frames"""
    sc, pipe = hd
    m, c = pipe.detect_device(sc.ptr(0), sc.w, sc.h, PIPE_N)
    check_rows(sc, m, c, 0, "detect_device")


def test_pipe_submit_collect_at_its_defaults(hd):
    """ocvar_hip_pipe_submit / _collect: 5 full chunks and a partial one through 4 contexts, oldest first; then Pipe.collect
    with max_frames below the chunk (the C call writes one row per frame of the chunk: the wrapper sizes for chunk_frames)"""
    sc, pipe = hd
    sizes = [2048] * 5 + [700]
    starts = [1031 * k for k in range(len(sizes))]   # (overlapping chunks of the device array: it is only read)
    sub = done = 0
    while done < len(sizes):
        while sub < len(sizes) and pipe.submit(sc.ptr(int(starts[sub])), sc.w, sc.h, sizes[sub], tag=sub):
            sub += 1
        tag, m, c = pipe.collect(2048)
        assert tag == done and len(c) == sizes[done]
        check_rows(sc, m, c, int(starts[done]), f"submit/collect chunk {done}")
        done += 1
    assert pipe.in_flight() == 0
    assert pipe.submit(sc.ptr(3), sc.w, sc.h, 2048, tag=99)
    tag, m, c = pipe.collect(16)
    assert tag == 99 and len(c) == 2048
    check_rows(sc, m, c, 3, "collect(16)")


def test_pipe_track_device_at_its_defaults(oa, hd):
    """ocvar_hip_pipe_track_device, two steps over 5820 streams (4 ragged chunks and a partial one): the frames are shifted on
    the device between the steps and the oracle is given the previous step's markers"""
    import torch
    sc, pipe = hd
    n = 512 + 1024 + 1536 + 2048 + 700
    m, c = pipe.track_device(sc.ptr(0), sc.w, sc.h, n, reset=True)
    check_rows(sc, m, c, 0, "track_device step 0")
    shifted_base = torch.roll(sc.d_base, shifts=(5, -4), dims=(1, 2))
    moved = shifted_base[torch.arange(n, device="cuda") % sc.U].contiguous()
    torch.cuda.synchronize()
    refs2 = oracle_all(shifted_base.cpu().numpy(), sc.tpls, sc.cam, prev=[r.markers for r in sc.refs], planes=False)
    m, c = pipe.track_device(moved.data_ptr(), sc.w, sc.h, n)
    for p in range(n):
        check_markers(p, refs2[p % sc.U], m, c, where=f"track_device step 1 stream {p}")
    assert sum(len(refs2[p % sc.U].markers) for p in range(n)) >= n
    del moved, shifted_base
    torch.cuda.empty_cache()


def test_pipe_result_limit_of_one_call_does_not_clamp_later_collects(oa, hd):
    """detect_device(max_per_frame=1) brings back one record per frame for that call only: a later submit / collect(64) gets every
    record of frames with 2-3 markers.  A collect asking for more records than set_result_limit brings back is refused and
    the chunk stays in flight."""
    import torch
    sc, pipe = hd
    multi = [u for u in range(sc.U) if 2 <= len(sc.refs[u].markers) <= 3]
    assert len(multi) >= 8
    j = [u + sc.U * k for k in range(8) for u in multi][:256]   # positions in the device array holding those frames
    n = len(j)
    m1, c1 = pipe.detect_device(sc.ptr(0), sc.w, sc.h, 600, max_per_frame=1)
    check_rows(sc, m1, c1, 0, "detect_device(max_per_frame=1)")
    sel = sc.d[torch.tensor(j, device="cuda")].contiguous()
    torch.cuda.synchronize()
    assert pipe.submit(sel.data_ptr(), sc.w, sc.h, n, tag=5)
    tag, m, c = pipe.collect(n, 64)
    assert tag == 5
    for p in range(n):
        u = j[p] % sc.U
        check_markers(p, sc.refs[u], m, c, where=f"collect(64) after detect_device(max_per_frame=1) position {p} frame {u}")
    pipe.set_result_limit(2)
    assert pipe.submit(sel.data_ptr(), sc.w, sc.h, n, tag=6)
    with pytest.raises(oa.OcvarError):
        pipe.collect(n, 64)
    assert pipe.in_flight() == 1
    tag, m, c = pipe.collect(n, 2)
    assert tag == 6
    for p in range(n):
        check_markers(p, sc.refs[j[p] % sc.U], m, c, where=f"collect(2) position {p}")
    pipe.set_result_limit(64)
    del sel

#!/usr/bin/env python3
"""What the kernels of ocvar_hip_flow_records (opencv-ar_amd/csrc/flow.hip) reach on this GPU, alone: frames/s and bytes/s of the
pyramid build at 1920x1080, BGR and grey, 256 frame pairs, and records/s of the track kernel at 16 records per frame with the default
parameters, next to what tools/hbm_ceiling.py reaches for a plain copy on the same box.  Not a test: there is no pass mark.

Every step (each format, the ceiling) runs in a process of its own under its own time limit; the first step that fails or runs
out of time ends the run.  A step warms up, then times REPS calls with device events and reports the median (and the best).  The
entry point has no pyramids-only form: a call whose counts are all 0 builds both pyramids of every frame pair and tracks nothing,
and the track kernel's time is a call with 16 live records per frame minus that.  Frame t + 1 is frame t moved by (3, 2) px, a
smooth texture: every corner converges as on a video.  Bytes of the pyramid build are the ones the definition needs: every frame
byte read once, every level written once, every level but the last read once."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, PER = 1920, 1080, 256, 16
WARMUP, REPS = 3, 15
STEP_SECONDS = {"bgr": 240, "gray": 240, "ceiling": 240}


def step(fmt):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=32)
    rng = np.random.default_rng(0)
    small = torch.from_numpy(rng.uniform(0, 255, (1, 1, H // 8 + 2, W // 8 + 2)).astype(np.float32)).cuda()
    base = torch.nn.functional.interpolate(small, scale_factor=8, mode="bicubic")[0, 0, :H, :W].clamp(0, 255).to(torch.uint8)
    frames = torch.empty((N + 1, H, W, bpp), dtype=torch.uint8, device="cuda")
    for t in range(N + 1):
        frames[t] = torch.roll(base, (2 * t, 3 * t), (0, 1))[..., None]
    sq = []
    for k in range(PER):
        x, y = 200 + 400 * (k % 4), 150 + 220 * (k // 4)
        sq.append([x, y, x + 120, y + 6, x + 114, y + 120, x - 6, y + 112])
    recs = np.zeros((N, PER), oa.MARKER_DTYPE)
    recs["square"] = np.asarray(sq, np.float32)
    recs["score"] = 1.0
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
    d_out = torch.empty_like(d_recs)
    d_status = torch.zeros(N * PER, dtype=torch.int32, device="cuda")
    counts = {0: torch.zeros(N, dtype=torch.int32, device="cuda"), PER: torch.full((N,), PER, dtype=torch.int32, device="cuda")}
    stream = torch.cuda.ExternalStream(det.stream_ptr())
    frame_bytes = H * W * bpp

    def timed(live):
        def launch():
            det.flow_records(frames.data_ptr(), frames.data_ptr() + frame_bytes, W, H, N, d_recs.data_ptr(), counts[live].data_ptr(), d_out.data_ptr(),
                             per_frame=PER, fmt=fmt, d_status_ptr=d_status.data_ptr())
        for _ in range(WARMUP):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return statistics.median(times), min(times)

    pyr_med, pyr_best = timed(0)
    assert int(d_status.count_nonzero()) == 0
    all_med, all_best = timed(PER)
    tracked = int((d_status == 1).sum())
    levels = [(W, H)]
    for _ in range(3):
        levels.append(((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2))
    px = [w * h for w, h in levels]
    nbytes = 2 * N * (frame_bytes + sum(px) + sum(px[:-1]))
    print(f"flow pyramids {W}x{H} {fmt}, {N} frame pairs, levels 0..3: median {pyr_med * 1e3:.3f} ms of {REPS} calls = {2 * N / pyr_med:.0f} frames/s, "
          f"{nbytes / pyr_med / 1e9:.0f} GB/s read + write (best {pyr_best * 1e3:.3f} ms = {nbytes / pyr_best / 1e9:.0f} GB/s)", flush=True)
    track = max(all_med - pyr_med, 1e-9)
    print(f"flow track {fmt}: {N} x {PER} records, {tracked} tracked: whole call median {all_med * 1e3:.3f} ms (best {all_best * 1e3:.3f} ms), "
          f"less the pyramids {track * 1e3:.3f} ms = {N * PER / track:.0f} records/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS))
    a = ap.parse_args()
    if a.step in ("bgr", "gray"):
        return step(a.step)
    for name, seconds in STEP_SECONDS.items():
        cmd = [sys.executable, os.path.join(ROOT, "tools", "hbm_ceiling.py")] if name == "ceiling" else [sys.executable, __file__, "--step", name]
        try:
            rc = subprocess.run(cmd, timeout=seconds).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {name} ended with status {rc}: nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the frame kernel of ocvar_hip_undistort (opencv-ar_amd/csrc/undistort.hip) reaches on this GPU, alone: frames/s and
bytes/s at 1920x1080, BGR and grey, 256 resident frames, next to what tools/hbm_ceiling.py reaches for a plain copy on the same
box.  Not a test: there is no pass mark.

Every step (each format, the ceiling) runs in a process of its own under its own time limit; the first step that fails or runs
out of time ends the run.  A step warms up, then times REPS launches with device events and reports the median (and the best).
Bytes are the ones the definition needs: every source byte read once, every destination byte written once."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [-0.21, 0.09, 0.0015, -0.0008, -0.02]   # k1 k2 p1 p2 k3: the barrel lens of the tests
W, H, N = 1920, 1080, 256
WARMUP, REPS = 5, 30
STEP_SECONDS = {"bgr": 180, "gray": 180, "ceiling": 240}


def step(fmt):
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=1)
    cam = oa.default_camera(W, H)
    cam.distCoeffs[:] = LENS
    det.set_camera(cam)
    src = torch.empty(N * H * W * bpp, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    dst = torch.empty_like(src)
    stream = torch.cuda.ExternalStream(det.stream_ptr())

    def launch():
        det.undistort(src.data_ptr(), dst.data_ptr(), W, H, N, fmt=fmt)

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
    assert int(dst.view(torch.int32).count_nonzero()) > 0   # (the kernel ran)
    nbytes = 2 * N * H * W * bpp
    med, best = statistics.median(times), min(times)
    print(f"undistort {W}x{H} {fmt} x {N}: median {med * 1e3:.3f} ms of {REPS} launches = {N / med:.0f} frames/s, "
          f"{nbytes / med / 1e9:.0f} GB/s read + write (best {best * 1e3:.3f} ms = {nbytes / best / 1e9:.0f} GB/s)", flush=True)


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

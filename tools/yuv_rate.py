#!/usr/bin/env python3
"""What the kernels of ocvar_hip_yuv_to_frames / ocvar_hip_frames_to_yuv (opencv-ar_amd/csrc/yuv.hip) reach on this GPU, alone:
NV12 -> BGR, NV12 -> GRAY and BGR -> NV12 at 1920x1080 with 64 frames resident, on the aligned path, in bytes moved per second
(source plus destination), next to what tools/hbm_ceiling.py reaches for a plain device copy in the same run on the same box.
The yardstick is that copy: a conversion below half of it has fallen off the wide path (the last line says so, and the exit
status is 1).

Every step (each conversion, the ceiling) runs in a process of its own under its own time limit; the first step that fails or
runs out of time ends the run.  A step warms up, then times REPS windows of INNER launches with device events and reports the median (and
the best) per launch.  Bytes are the ones the definition needs: every source byte read once, every destination byte written once."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 64
WARMUP, REPS, INNER = 10, 30, 20   # a timed window is INNER launches back to back (a single one lasts about 0.1 ms)
STEPS = {"nv12-bgr": ("bgr", True), "nv12-gray": ("gray", True), "bgr-nv12": ("bgr", False)}
STEP_SECONDS = 180
FLOOR = 0.5


def step(name):
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    fmt, to_frames = STEPS[name]
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=1)
    yuv = torch.empty(N * H * W * 3 // 2, dtype=torch.uint8, device="cuda")
    pix = torch.empty(N * H * W * bpp, dtype=torch.uint8, device="cuda")
    (yuv if to_frames else pix).random_(0, 255)
    (pix if to_frames else yuv).zero_()
    st = oa.YuvFrames.from_surface(yuv.data_ptr(), W, H, "nv12")
    stream = torch.cuda.ExternalStream(det.stream_ptr())

    def launch():
        if to_frames:
            det.yuv_to_frames(st, pix.data_ptr(), W, H, N, fmt=fmt)
        else:
            det.frames_to_yuv(pix.data_ptr(), st, W, H, N, fmt=fmt)

    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(INNER):
            launch()
        e1.record(stream)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3 / INNER)
    assert int((pix if to_frames else yuv).view(torch.int32).count_nonzero()) > 0   # (the kernel ran)
    nbytes = N * H * W * 3 // 2 + N * H * W * bpp
    med, best = statistics.median(times), min(times)
    print(f"yuv {name} {W}x{H} x {N}: median {med * 1e3:.3f} ms per launch over {REPS} windows of {INNER} = {N / med:.0f} frames/s, "
          f"{nbytes / med / 1e9:.0f} GB/s read + write (best {best * 1e3:.3f} ms = {nbytes / best / 1e9:.0f} GB/s)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    rates, copy = {}, None
    for name in list(STEPS) + ["ceiling"]:
        cmd = [sys.executable, os.path.join(ROOT, "tools", "hbm_ceiling.py")] if name == "ceiling" else [sys.executable, __file__, "--step", name]
        try:
            r = subprocess.run(cmd, timeout=STEP_SECONDS, capture_output=True, text=True)
            rc = r.returncode
            sys.stdout.write(r.stdout)
            sys.stderr.write(r.stderr[-2000:])
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {name} ended with status {rc}: nothing more is started", flush=True)
            return rc
        if name == "ceiling":
            copy = float(re.search(r"copy .*: (\d+) GB/s", r.stdout).group(1))
        else:
            rates[name] = float(re.search(r"(\d+) GB/s read \+ write \(best", r.stdout).group(1))
    ratios = {k: v / copy for k, v in rates.items()}
    print("of the plain copy's %.0f GB/s: %s (floor %.2f)" % (copy, ", ".join("%s %.2f" % kv for kv in ratios.items()), FLOOR), flush=True)
    missed = [k for k, v in ratios.items() if v < FLOOR]
    if missed:
        print("BELOW THE FLOOR: " + ", ".join(missed), flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

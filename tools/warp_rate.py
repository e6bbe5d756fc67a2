#!/usr/bin/env python3
"""What the frame kernel of ocvar_hip_warp (opencv-ar_amd/csrc/warp.hip) reaches on this GPU, alone: frames/s and bytes/s at
1920x1080, BGR and grey, 256 resident frames, LINEAR with a CONSTANT border under a mild map (a turn of 5 degrees about the centre
with a slight perspective), with its tiles staged through LDS and with every tile made direct by the tuning switch
(OCVAR_TUNE_WARP_DIRECT) -- next to ocvar_hip_undistort with the tests' barrel lens, the other full-frame gather, and to what
tools/hbm_ceiling.py reaches for a plain device copy, all in one run on the same box.  Two conditions, and exit status 1 when one
is missed: the warp (fewer operations per pixel than the lens model, the same four taps) is no slower per destination pixel than
undistort in either format; and the staged class beats the all-direct run of the same map -- a second path that buys nothing is
not kept.

Every step runs in a process of its own under its own time limit; the first step that fails or runs out of time ends the run.
A step warms up, then times REPS launches with device events and reports the median (and the best).  Bytes are the ones the
definition needs: every source byte read once, every destination byte written once (source and destination have the same size)."""
import argparse
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [-0.21, 0.09, 0.0015, -0.0008, -0.02]   # k1 k2 p1 p2 k3: the barrel lens of the tests
W, H, N = 1920, 1080, 256
WARMUP, REPS = 5, 30
STEPS = ["undistort-bgr", "undistort-gray", "warp-bgr", "warp-gray", "direct-bgr", "direct-gray"]
STEP_SECONDS = 180


def mild_map():
    """the forward map: the source turned by 5 degrees about its centre, perspective terms 2e-5 and -1e-5 per pixel"""
    import numpy as np
    a = math.radians(5.0)
    T0 = np.array([[1, 0, -(W - 1) / 2], [0, 1, -(H - 1) / 2], [0, 0, 1.0]])
    A = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [2e-5, -1e-5, 1.0]])
    T1 = np.array([[1, 0, (W - 1) / 2], [0, 1, (H - 1) / 2], [0, 0, 1.0]])
    return (T1 @ A @ T0).reshape(9)


def step(name):
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    what, fmt = name.split("-")
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=1)
    cam = oa.default_camera(W, H)
    cam.distCoeffs[:] = LENS
    det.set_camera(cam)
    src = torch.empty(N * H * W * bpp, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    dst = torch.empty_like(src)
    maps = torch.from_numpy(mild_map()).to("cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(det.stream_ptr())
    if what == "direct":
        det.set_tuning(warp_direct=1)

    def launch():
        if what == "undistort":
            det.undistort(src.data_ptr(), dst.data_ptr(), W, H, N, fmt=fmt)
        else:
            det.warp(src.data_ptr(), W, H, dst.data_ptr(), W, H, N, maps.data_ptr(), one_map=True, fmt=fmt, d_status_ptr=status.data_ptr())

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
    assert what == "undistort" or int(status.sum()) == N
    nbytes = 2 * N * H * W * bpp
    med, best = statistics.median(times), min(times)
    print(f"{name} {W}x{H} x {N}: median {med * 1e3:.3f} ms of {REPS} launches = {N / med:.0f} frames/s, {N * W * H / med / 1e9:.2f} Gpx/s, "
          f"{nbytes / med / 1e9:.0f} GB/s read + write (best {best * 1e3:.3f} ms = {nbytes / best / 1e9:.0f} GB/s)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    ms, gbs, copy = {}, {}, None
    for name in STEPS + ["ceiling"]:
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
            ms[name] = float(re.search(r"median ([\d.]+) ms", r.stdout).group(1))
            gbs[name] = float(re.search(r"(\d+) GB/s read \+ write \(best", r.stdout).group(1))
    print("of the plain copy's %.0f GB/s: %s" % (copy, ", ".join("%s %.2f" % (k, v / copy) for k, v in gbs.items())), flush=True)
    missed = []
    for fmt in ("bgr", "gray"):
        u, w, d = ms["undistort-" + fmt], ms["warp-" + fmt], ms["direct-" + fmt]
        print("%s: warp / undistort %.2f of the time per destination pixel (%.3f ms against %.3f ms); staged / all direct %.2f (%.3f ms against %.3f ms)" % (
            fmt, w / u, w, u, w / d, w, d), flush=True)
        if w > u:
            missed.append("warp-%s is slower than undistort-%s" % (fmt, fmt))
        if w >= d:
            missed.append("staging buys nothing in %s" % fmt)
    if missed:
        print("MISSED: " + "; ".join(missed), flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

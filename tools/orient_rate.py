#!/usr/bin/env python3
"""What the kernels of ocvar_hip_orient (opencv-ar_amd/csrc/orient.hip) reach on this GPU, alone, with 32 frames resident on the
aligned path: 1920x1080 FLIP_H in BGR and in GRAY and ROT180 in BGR (the row-reversing kernels), 1920x1080 ROT90_CW in BGR, GRAY
and BGRA and 3840x2160 ROT90_CW in BGR (the transposing kernel), in bytes moved per second (source plus destination), next to
what tools/hbm_ceiling.py reaches for a plain device copy in the same run on the same box.  The yardstick is that copy, for the
three row-reversing steps: a pure streaming pass below half of it has fallen off the wide path (the last line says so, and the
exit status is 1).  The transposing steps are reported without a floor.

Every step (each orientation, the ceiling) runs in a process of its own under its own time limit; the first step that fails or
runs out of time ends the run.  A step warms up, then times REPS windows of INNER launches with device events and reports the
median (and the best) per launch.  Bytes are the ones the definition needs: every source byte read once, every destination byte
written once."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 32
WARMUP, REPS, INNER = 10, 30, 20   # a timed window is INNER launches back to back (a single one lasts a fraction of a ms)
# name: (format, orientation, source size, held to the floor)
STEPS = {"flip_h-bgr": ("bgr", "flip_h", (1920, 1080), True),
         "flip_h-gray": ("gray", "flip_h", (1920, 1080), True),
         "rot180-bgr": ("bgr", "rot180", (1920, 1080), True),
         "rot90-bgr": ("bgr", "rot90", (1920, 1080), False),
         "rot90-gray": ("gray", "rot90", (1920, 1080), False),
         "rot90-bgra": ("bgra", "rot90", (1920, 1080), False),
         "rot90-bgr-4k": ("bgr", "rot90", (3840, 2160), False)}
STEP_SECONDS = 180
FLOOR = 0.5   # tools/yuv_rate.py


def step(name):
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    fmt, orientation, (sw, sh), _ = STEPS[name]
    dw, dh = oa.oriented_size((sw, sh), orientation)
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(64, 64, max_batch=1)   # (the sizes are not bound by the context's)
    src = torch.empty(N * sh * sw * bpp, dtype=torch.uint8, device="cuda")
    dst = torch.empty(N * dh * dw * bpp, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    dst.zero_()
    assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0 and (sw * bpp) % 4 == 0 and (dw * bpp) % 4 == 0   # the aligned path
    stream = torch.cuda.ExternalStream(det.stream_ptr())

    def launch():
        det.orient(src.data_ptr(), sw, sh, dst.data_ptr(), N, orientation, fmt=fmt)

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
    assert int(dst.view(torch.int32).count_nonzero()) > 0   # (the kernel ran)
    nbytes = N * bpp * (sw * sh + dw * dh)
    med, best = statistics.median(times), min(times)
    print(f"orient {name} {sw}x{sh} -> {dw}x{dh} x {N}: median {med * 1e3:.3f} ms per launch over {REPS} windows of {INNER} = {N / med:.0f} frames/s, "
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
    print("of the plain copy's %.0f GB/s: %s (floor %.2f for %s)" % (
        copy, ", ".join("%s %.2f" % kv for kv in ratios.items()), FLOOR, ", ".join(k for k in STEPS if STEPS[k][3])), flush=True)
    missed = [k for k, v in ratios.items() if STEPS[k][3] and v < FLOOR]
    if missed:
        print("BELOW THE FLOOR: " + ", ".join(missed), flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

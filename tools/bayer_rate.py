#!/usr/bin/env python3
"""What the kernels of ocvar_hip_bayer_to_frames (opencv-ar_amd/csrc/bayer.hip) reach on this GPU, alone: 8-bit and 12-bit-in-16
RGGB mosaics -> BGR and -> GRAY at 1920x1080 with 64 (or --frames 256) frames resident, on the aligned path, in bytes moved per
second (source plus destination); -> BGR also with lanes that march down 1, 2 and 16 row pairs instead of the default
(OCVAR_TUNE_BAYER_PAIRS; 1 is the kernel without the march: four source rows loaded and balanced for every pair); next to the
nearest existing kernel, ocvar_hip_yuv_to_frames NV12 -> BGR (the same bytes written, 1.5 times the bytes read of the 8-bit
mosaic), and to what tools/hbm_ceiling.py reaches for a plain device copy, all in the same run on the same box.  The last line gives every rate as a share of that copy; no rate is fixed in advance, the number to hold
Bayer -> BGR against is NV12 -> BGR's share.

Every step (each conversion, the ceiling) runs in a process of its own under its own time limit; the first step that fails or
runs out of time ends the run.  A step warms up, then times REPS windows of INNER launches with device events and reports the median
(and the best) per launch.  Bytes are the ones the definition needs: every source byte read once, every destination byte written
once (the kernels read the two source rows at a strip's ends a second time and each lane two halo samples per row; neither is
counted).  The parameters are non-default (a black level, three different gains): the arithmetic is the same for the defaults."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
WARMUP, REPS, INNER = 10, 30, 20   # a timed window is INNER launches back to back
# step -> (source: bits of a mosaic or "nv12", destination format, row pairs a lane marches down -- 0: the library's default)
STEPS = {"bayer8-bgr": (8, "bgr", 0), "bayer8-gray": (8, "gray", 0), "bayer12-bgr": (12, "bgr", 0), "bayer12-gray": (12, "gray", 0),
         "bayer8-bgr-pairs1": (8, "bgr", 1), "bayer8-bgr-pairs2": (8, "bgr", 2), "bayer8-bgr-pairs16": (8, "bgr", 16),
         "bayer12-bgr-pairs1": (12, "bgr", 1), "bayer12-bgr-pairs16": (12, "bgr", 16), "nv12-bgr": ("nv12", "bgr", 0)}
STEP_SECONDS = 180


def step(name, n):
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    source, fmt, pairs = STEPS[name]
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=1)
    if pairs:
        det.set_tuning(bayer_pairs=pairs)
    src_bytes = n * H * W * 3 // 2 if source == "nv12" else n * H * W * (2 if source > 8 else 1)
    src = torch.empty(src_bytes, dtype=torch.uint8, device="cuda")
    pix = torch.empty(n * H * W * bpp, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    pix.zero_()
    stream = torch.cuda.ExternalStream(det.stream_ptr())
    if source == "nv12":
        st = oa.YuvFrames.from_surface(src.data_ptr(), W, H, "nv12")

        def launch():
            det.yuv_to_frames(st, pix.data_ptr(), W, H, n, fmt=fmt)
    else:
        p = oa.bayer_params("rggb", source, 16 if source == 8 else 256, (1.6, 1.0, 1.9))

        def launch():
            det.bayer_to_frames(src.data_ptr(), pix.data_ptr(), W, H, n, params=p, fmt=fmt)

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
    assert int(pix.view(torch.int32).count_nonzero()) > 0   # (the kernel ran)
    nbytes = src_bytes + n * H * W * bpp
    med, best = statistics.median(times), min(times)
    print(f"{name} {W}x{H} x {n}: median {med * 1e3:.3f} ms per launch over {REPS} windows of {INNER} = {n / med:.0f} frames/s, "
          f"{nbytes / med / 1e9:.0f} GB/s read + write (best {best * 1e3:.3f} ms = {nbytes / best / 1e9:.0f} GB/s)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--frames", type=int, choices=[64, 256], default=64)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.frames)
    rates, copy = {}, None
    for name in list(STEPS) + ["ceiling"]:
        cmd = [sys.executable, os.path.join(ROOT, "tools", "hbm_ceiling.py")] if name == "ceiling" else [
            sys.executable, __file__, "--step", name, "--frames", str(a.frames)]
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
    print("of the plain copy's %.0f GB/s: %s" % (copy, ", ".join("%s %.2f" % (k, v / copy) for k, v in rates.items())), flush=True)
    print("Bayer -> BGR against NV12 -> BGR: 8-bit %.2f, 12-bit %.2f of its rate" % (
        rates["bayer8-bgr"] / rates["nv12-bgr"], rates["bayer12-bgr"] / rates["nv12-bgr"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

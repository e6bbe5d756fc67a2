#!/usr/bin/env python3
"""What the kernels of ocvar_hip_yuv_to_frames_ex / ocvar_hip_frames_to_yuv_ex (opencv-ar_amd/csrc/yuv_ex.hip) reach on this GPU,
alone: P010 -> BGR, P010 -> GRAY, full-range NV12 -> BGR, I444 -> BGR and BGR -> P010 at 1920x1080 with 64 frames resident, on
the aligned path, next to NV12 -> BGR through the old entry point and to a plain device copy of 2 GiB, all in one run on the
same box.  A rate is bytes moved per second: every source byte read once, every destination byte written once.  Each conversion
is reported as a fraction of the copy's rate, median over median and best over best.

Every step runs in a process of its own under its own time limit; the first step that fails or runs out of time ends the run.
A step warms up, then times REPS windows of INNER launches with device events and reports the median (and the best) per
launch."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 64
WARMUP, REPS, INNER = 10, 30, 20   # a timed window is INNER launches back to back (a single one lasts about 0.1 ms)
COPY_BYTES, COPY_INNER = 2 << 30, 2
# step -> (layout, bits, range, matrix, format, to_frames, through the old entry point)
STEPS = {"p010-bgr": ("nv12", 10, "limited", "bt709", "bgr", True, False), "p010-gray": ("nv12", 10, "limited", "bt709", "gray", True, False),
         "nv12full-bgr": ("nv12", 8, "full", "bt601", "bgr", True, False), "i444-bgr": ("i444", 8, "full", "bt601", "bgr", True, False),
         "bgr-p010": ("nv12", 10, "limited", "bt709", "bgr", False, False), "nv12-bgr-old": ("nv12", 8, "limited", "bt601", "bgr", True, True)}
STEP_SECONDS = 180


def timed(launch, stream, inner):
    import torch
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            launch()
        e1.record(stream)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3 / inner)
    return statistics.median(times), min(times)


def report(name, what, nbytes, med, best):
    print(f"{name} {what}: median {med * 1e3:.3f} ms per launch over {REPS} windows = {nbytes / med / 1e9:.0f} GB/s read + write "
          f"(best {best * 1e3:.3f} ms = {nbytes / best / 1e9:.0f} GB/s)", flush=True)


def copy_step():
    import torch
    a = torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda")
    b = torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda")
    a.random_(0, 255)
    med, best = timed(lambda: b.copy_(a), torch.cuda.current_stream(), COPY_INNER)
    report("copy", "2 GiB", 2 * COPY_BYTES, med, best)


def step(name):
    import torch
    if name == "copy":
        return copy_step()
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    layout, bits, rng, matrix, fmt, to_frames, old = STEPS[name]
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=1)
    yuv_bytes = N * H * W * 3 // (1 if layout == "i444" or bits > 8 else 2)   # 3 bytes per pixel in I444 and P010, 1.5 in NV12
    yuv = torch.empty(yuv_bytes, dtype=torch.uint8, device="cuda")
    pix = torch.empty(N * H * W * bpp, dtype=torch.uint8, device="cuda")
    (yuv if to_frames else pix).random_(0, 255)
    (pix if to_frames else yuv).zero_()
    if old:
        st = oa.YuvFrames.from_surface(yuv.data_ptr(), W, H, layout, matrix=matrix)
    else:
        st = oa.YuvFramesEx.from_surface(yuv.data_ptr(), W, H, layout, matrix=matrix, range=rng, bits=bits)
    assert st.frame_stride * N == yuv_bytes
    stream = torch.cuda.ExternalStream(det.stream_ptr())

    def launch():
        if to_frames:
            det.yuv_to_frames(st, pix.data_ptr(), W, H, N, fmt=fmt)
        else:
            det.frames_to_yuv(pix.data_ptr(), st, W, H, N, fmt=fmt)

    med, best = timed(launch, stream, INNER)
    assert int((pix if to_frames else yuv).view(torch.int32).count_nonzero()) > 0   # (the kernel ran)
    report(name, f"{W}x{H} x {N}", yuv_bytes + N * H * W * bpp, med, best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS) + ["copy"])
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    rates = {}
    for name in list(STEPS) + ["copy"]:
        try:
            r = subprocess.run([sys.executable, __file__, "--step", name], timeout=STEP_SECONDS, capture_output=True, text=True)
            rc = r.returncode
            sys.stdout.write(r.stdout)
            sys.stderr.write(r.stderr[-2000:])
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {name} ended with status {rc}: nothing more is started", flush=True)
            return rc
        m = re.search(r"= (\d+) GB/s read \+ write \(best .* = (\d+) GB/s\)", r.stdout)
        rates[name] = (float(m.group(1)), float(m.group(2)))
    copy = rates.pop("copy")
    print("of the plain copy's %.0f GB/s (best %.0f): %s" % (copy[0], copy[1], ", ".join(
        "%s %.2f (best %.2f)" % (k, v[0] / copy[0], v[1] / copy[1]) for k, v in rates.items())), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

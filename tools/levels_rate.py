#!/usr/bin/env python3
"""What ocvar_hip_levels (opencv-ar_amd/csrc/levels.hip) reaches on this GPU, alone, with 256 resident 1920x1080 frames on the
aligned path: BGR and GRAY sources, grids of 1x1, 4x4 and 8x8 tiles, on synthetic scenes and on a constant frame (every lane of the
histogram kernel on one bin), next to a plain device copy of the same source bytes in the same run; then each of the three
kernels on its own, from a kernel trace taken in a run of its own.  Bytes are the ones the definition needs: every source byte read
twice (histogram, apply), one destination byte per pixel written; the copy's are its bytes read plus its bytes written.  Each time
is given in milliseconds and as a fraction of the copy's bytes per second.  No rate is promised: the last lines say what the numbers
show, and whether the constant frame is pathologically slower than a scene (more than PATHOLOGICAL times: exit status 1).

Every step runs in a process of its own under its own time limit; the first step that fails or runs out of time ends the run.  A
step warms up, then times REPS windows of INNER launches with device events and reports the median (and the best) per launch."""
import argparse
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, H = 256, 1920, 1080
WARMUP, REPS, INNER = 3, 10, 4      # (a launch lasts of the order of a millisecond)
FORMATS = ("bgr", "gray")
GRIDS = ((1, 1), (4, 4), (8, 8))
CONTENTS = ("scene", "constant")
DISTINCT = 8                        # synthetic scenes, repeated through the 256 frames
STEP_SECONDS = 240
PATHOLOGICAL = 3.0
KERNELS = ("levels_hist_kernel", "levels_lut_kernel", "levels_apply_kernel")


def step_name(fmt, grid, content):
    return "%s-%dx%d-%s" % (fmt, grid[0], grid[1], content)


STEPS = {step_name(f, g, c): (f, g, c) for f in FORMATS for g in GRIDS for c in CONTENTS}


def frames(fmt, content):
    """the N source frames on the device: [N, H, W, 3] BGR or [N, H, W] GRAY"""
    import numpy as np
    import torch
    if content == "constant":
        shape = (N, H, W, 3) if fmt == "bgr" else (N, H, W)
        return torch.full(shape, 128, dtype=torch.uint8, device="cuda")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    cfg = Hh.synth_config(3)
    assert (cfg.width, cfg.height) == (W, H)
    bgr = np.stack([Hh.synth_frame(cfg, f)[0] for f in range(DISTINCT)])
    if fmt == "gray":
        b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
        bgr = ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)
    d = torch.from_numpy(bgr).cuda()
    return d.repeat((N // DISTINCT,) + (1,) * (d.dim() - 1)).contiguous()


def timed(launch, stream):
    import torch
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
    return statistics.median(times), min(times)


def step(name, launches=None):
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    fmt, grid, content = STEPS[name]
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(64, 64, max_batch=1)   # (the sizes are not bound by the context's)
    src = frames(fmt, content)
    dst = torch.zeros(N * H * W, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0 and (W * bpp) % 4 == 0   # the aligned path
    p = oa.levels_params(tiles=grid)
    stream = torch.cuda.ExternalStream(det.stream_ptr())

    def launch():
        det.levels(src.data_ptr(), dst.data_ptr(), W, H, N, params=p, fmt=fmt)

    if launches is not None:      # under the kernel trace: a few launches, no timing of our own
        for _ in range(launches):
            launch()
        torch.cuda.synchronize()
        return
    med, best = timed(launch, stream)
    assert int(dst.view(torch.int32).count_nonzero()) > 0   # (the kernels ran)
    nbytes = N * W * H * (2 * bpp + 1)
    print(f"levels {name} {W}x{H} x {N}: median {med * 1e3:.3f} ms per launch over {REPS} windows of {INNER} = {N / med:.0f} frames/s, "
          f"{nbytes / med / 1e9:.0f} GB/s of the definition's bytes (best {best * 1e3:.3f} ms = {nbytes / best / 1e9:.0f} GB/s)", flush=True)


def copy_step(fmt):
    import torch
    bpp = 3 if fmt == "bgr" else 1
    src = torch.empty(N * H * W * bpp, dtype=torch.uint8, device="cuda")
    src.random_(0, 255)
    dst = torch.empty_like(src)
    med, best = timed(lambda: dst.copy_(src), torch.cuda.current_stream())
    nbytes = 2 * src.numel()
    print(f"copy {fmt} {src.numel()} bytes: median {med * 1e3:.3f} ms = {nbytes / med / 1e9:.0f} GB/s read + write (best {best * 1e3:.3f} ms = "
          f"{nbytes / best / 1e9:.0f} GB/s)", flush=True)


def kernel_times(name, out_dir):
    """the step under rocprofv3's kernel trace, in a run of its own -> {kernel: (mean ms, launches)} over the launches after the first"""
    launches = 4
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--", sys.executable, __file__, "--step", name, "--launches", str(launches)]
    r = subprocess.run(cmd, timeout=STEP_SECONDS, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        return None
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    out = {}
    for k in KERNELS:
        t = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows if k in r["Kernel_Name"])
        t = [d for _, d in t[len(t) // launches:]]      # (the first launch's kernels load the code object)
        if t:
            out[k] = (statistics.mean(t) * 1e-6, len(t))
    return out


def run(cmd):
    try:
        r = subprocess.run(cmd, timeout=STEP_SECONDS, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        return 124, ""
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr[-2000:])
    return r.returncode, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--copy", choices=FORMATS)
    ap.add_argument("--launches", type=int)
    ap.add_argument("--trace-dir", help="where the kernel traces go (default: a temporary directory)")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.launches)
    if a.copy:
        return copy_step(a.copy)
    trace_dir = a.trace_dir or tempfile.mkdtemp(prefix="levels_trace_")
    print(f"tools/levels_rate.py on one MI355X, alone: {N} resident {W}x{H} frames, aligned path, bytes = 2 x source + 1 per pixel", flush=True)
    copy, ms, rate = {}, {}, {}
    for fmt in FORMATS:
        rc, out = run([sys.executable, __file__, "--copy", fmt])
        if rc != 0:
            print(f"copy {fmt} ended with status {rc}: nothing more is started", flush=True)
            return rc
        copy[fmt] = float(re.search(r"= (\d+) GB/s read \+ write \(best", out).group(1))
    for name in STEPS:
        rc, out = run([sys.executable, __file__, "--step", name])
        if rc != 0:
            print(f"step {name} ended with status {rc}: nothing more is started", flush=True)
            return rc
        ms[name] = float(re.search(r"median ([\d.]+) ms", out).group(1))
        rate[name] = float(re.search(r"(\d+) GB/s of the definition's bytes \(best", out).group(1))
    for fmt in FORMATS:
        print("of the %s copy's %.0f GB/s: %s" % (fmt, copy[fmt], ", ".join(
            "%s %.3f ms %.2f" % (n, ms[n], rate[n] / copy[fmt]) for n in STEPS if STEPS[n][0] == fmt)), flush=True)
    worst = max(ms[step_name(f, g, "constant")] / ms[step_name(f, g, "scene")] for f in FORMATS for g in GRIDS)
    print("a constant frame takes at most %.2f times a scene's time (pathological: above %.1f)" % (worst, PATHOLOGICAL), flush=True)
    for fmt in FORMATS:
        for content in CONTENTS:
            name = step_name(fmt, (4, 4), content)
            kt = kernel_times(name, os.path.join(trace_dir, name))
            if not kt:
                print(f"kernel trace of {name}: not measured (the profiler's run failed or left no trace)", flush=True)
                continue
            bpp = 3 if fmt == "bgr" else 1
            kbytes = {KERNELS[0]: N * W * H * bpp, KERNELS[1]: 0, KERNELS[2]: N * W * H * (bpp + 1)}
            print("kernels of %s: %s" % (name, ", ".join("%s %.3f ms x %d%s" % (
                k.replace("levels_", "").replace("_kernel", ""), kt[k][0], kt[k][1],
                " = %.2f of the copy's rate" % (kbytes[k] / (kt[k][0] * 1e-3) / 1e9 / copy[fmt]) if kbytes[k] else "") for k in KERNELS if k in kt)), flush=True)
    return 1 if worst > PATHOLOGICAL else 0


if __name__ == "__main__":
    sys.exit(main())

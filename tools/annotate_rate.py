#!/usr/bin/env python3
"""What ocvar_hip_annotate_records (opencv-ar_amd/csrc/annotate.hip) reaches on this GPU next to its two yardsticks, in one run:
on 256 resident 1920x1080 frames of the bench's synthetic scenes (tests/helpers.synth_config(3): 16 planted markers a frame), in
BGR and in GRAY, with 16 records per frame (the planted corners, their poses solved by the oracle), it times
    copy       a plain device copy of the frames (every byte read once and written once)
    render     render_records with a 64 x 64 default overlay on those records (touches every pixel inside the quads)
    outline    annotate_records with outline + corner 0, the default thickness (touches the quads' rims)
    all        annotate_records with every flag on (outline, corner 0, cube, axes, label, unmatched, colour by template)
and reports frames per second for each, and the ratios outline / copy, outline / render, all / copy and all / render of those
rates.  The yardstick is the render of the same records: an outline that is not at least as fast as it means the per-primitive
culling is not working (the last line says so, and the exit status is 1).

Each format runs in a process of its own under its own time limit; the first that fails or runs out of time ends the run.  A
step warms up, then the four steps take turns: REPS rounds, in each a window of INNER launches per step, timed with device events;
the median per launch (and the best) is reported.  --out FILE also writes the report there."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, UNIQUE, PER_FRAME = 256, 32, 16
W, H = 1920, 1080
WARMUP, REPS, INNER = 3, 15, 4
STEP_SECONDS = 400
FORMATS = ("bgr", "gray")
STEPS = ("copy", "render", "outline", "all")


def scene_records():
    """(frames [UNIQUE, H, W, 3] uint8, records [UNIQUE, PER_FRAME], camera): the bench's scenes and a record per planted marker"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hp
    import opencv_ar_amd as oa
    cfg = Hp.synth_config(3)
    assert (cfg.width, cfg.height, cfg.grid_x * cfg.grid_y) == (W, H, PER_FRAME)
    cam = Hp.oracle_camera(W, H)
    frames = np.zeros((UNIQUE, H, W, 3), np.uint8)
    recs = np.zeros((UNIQUE, PER_FRAME), oa.MARKER_DTYPE)
    for f in range(UNIQUE):
        frames[f], truth = Hp.synth_frame(cfg, f)
        assert len(truth) == PER_FRAME
        for k, t in enumerate(truth):
            sq = np.ascontiguousarray((t["corner"] - 0.5).reshape(8), np.float32)   # (the generator's pixel (x, y) covers [x, x + 1))
            gl = np.zeros(16, np.float64)
            Hp.oracle().orc_square_to_matrix(Hp.P(sq), C.byref(cam), 1.0, Hp.P(gl))
            recs[f, k]["square"], recs[f, k]["glMatrix"] = sq, gl
            recs[f, k]["templateId"], recs[f, k]["markerId"], recs[f, k]["score"], recs[f, k]["aspectRatio"] = t["template"], k, 1.0, 1.0
    return frames, recs, cam


def step(fmt):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opencv_ar_amd as oa
    frames, recs, cam = scene_records()
    if fmt == "gray":
        f64 = frames.astype(np.int64)
        frames = ((1868 * f64[..., 0] + 9617 * f64[..., 1] + 4899 * f64[..., 2] + 8192) >> 14).astype(np.uint8)
    bpp = oa.FORMAT_BPP[oa.input_format_code(fmt)]
    det = oa.Detector(W, H, max_batch=N)
    det.set_camera(oa.Camera.from_buffer_copy(bytes(cam)))
    ov = np.zeros((64, 64, 4), np.uint8)
    ov[...] = (40, 200, 90, 255)
    ov[::8, :, :3] = 255
    det.set_overlay(-1, ov)
    reps = N // UNIQUE
    src = torch.from_numpy(frames.reshape(UNIQUE, -1)).to("cuda").repeat(reps, 1).reshape(-1).contiguous()
    dst = torch.empty_like(src)
    drecs = torch.from_numpy(recs.view(np.uint8).reshape(UNIQUE, -1)).to("cuda").repeat(reps, 1).reshape(-1).contiguous()
    dcounts = torch.full((N,), PER_FRAME, dtype=torch.int32, device="cuda")
    assert src.numel() == N * W * H * bpp and src.data_ptr() % 4 == 0 and (W * bpp) % 4 == 0   # the aligned path
    stream = torch.cuda.ExternalStream(det.stream_ptr())
    outline = oa.annotate_style(label=False)
    everything = oa.annotate_style(axes=True, cube=True, unmatched=True, color_by_template=True)

    def annotate(style):
        det.annotate_records(dst.data_ptr(), W, H, N, drecs.data_ptr(), dcounts.data_ptr(), per_frame=PER_FRAME, style=style, fmt=fmt)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src)

    launch = {"copy": copy,
              "render": lambda: det.render_records(dst.data_ptr(), W, H, N, drecs.data_ptr(), dcounts.data_ptr(), per_frame=PER_FRAME, fmt=fmt),
              "outline": lambda: annotate(outline), "all": lambda: annotate(everything)}
    copy()
    torch.cuda.synchronize()
    changed = {}
    for name in STEPS[1:]:   # (each step draws: the frames differ from the source afterwards)
        copy()
        launch[name]()
        torch.cuda.synchronize()
        changed[name] = int((dst != src).sum())
        assert changed[name] > 0, name
    for _ in range(WARMUP):
        for name in STEPS:
            launch[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in STEPS}
    for _ in range(REPS):
        for name in STEPS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(INNER):
                launch[name]()
            e1.record(stream)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3 / INNER)
    for name in STEPS:
        med, best = statistics.median(times[name]), min(times[name])
        extra = f", {2 * src.numel() / med / 1e9:.0f} GB/s read + write" if name == "copy" else f", {changed[name] / N:.0f} bytes changed per frame"
        print(f"annotate_rate {fmt} {name}: median {med * 1e3:.3f} ms per {N} frames of {W}x{H} over {REPS} windows of {INNER} = {N / med:.0f} frames/s "
              f"(best {best * 1e3:.3f} ms){extra}", flush=True)


def main():
    import re
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=FORMATS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    lines, rates = [f"tools/annotate_rate.py on one MI355X, alone: {N} resident {W}x{H} frames, {PER_FRAME} records per frame, aligned path"], {}
    for fmt in FORMATS:
        try:
            r = subprocess.run([sys.executable, __file__, "--step", fmt], timeout=STEP_SECONDS, capture_output=True, text=True)
            rc = r.returncode
            sys.stdout.write(r.stdout)
            sys.stderr.write(r.stderr[-2000:])
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"step {fmt} ended with status {rc}: nothing more is started", flush=True)
            return rc
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("annotate_rate ")]
        for name in STEPS:
            rates[fmt, name] = float(re.search(rf"annotate_rate {fmt} {name}: .* = (\d+) frames/s", r.stdout).group(1))
    slow = []
    for fmt in FORMATS:
        q = {f"{a_}/{b}": rates[fmt, a_] / rates[fmt, b] for a_ in ("outline", "all") for b in ("copy", "render")}
        lines.append(f"annotate_rate {fmt} ratios of frames/s: " + ", ".join(f"{k} {v:.2f}" for k, v in q.items()))
        print(lines[-1], flush=True)
        if q["outline/render"] < 1.0:
            slow.append(fmt)
    lines.append("OUTLINE SLOWER THAN THE OVERLAY RENDER: " + ", ".join(slow) if slow else "outline-only annotation is at least as fast as the overlay render of the same records")
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Cost of drawing overlays (ocvar_hip_render_records, the kernels of ocvar_hip_render) on the benchmark's frames: 256 distinct
1080p BGR frames of config 3 (16 markers each), one 256 x 256 overlay per template, against a plain device copy of the same
frames (tools/hbm_ceiling.py's pattern: best of 20, HIP events).  Two libraries: the benchmark's three templates (the
registration keeps one marker per template: 3 records per frame) and one template per marker (16 records per frame).
    python tools/overlay_rate.py [output file, default profiles/overlay_rate.txt]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import dense_synth as DS
import helpers as H
import opencv_ar_amd as oa

N = 256
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "overlay_rate.txt")
cfg = H.synth_config(3)
W, Hh = cfg.width, cfg.height
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def best(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return min(t), float(np.median(t))


say(f"{torch.cuda.get_device_name(0)}; {oa.build_info()}")
say(f"{N} distinct {W} x {Hh} BGR frames ({N * W * Hh * 3 / 1e6:.0f} MB), 256 x 256 overlays, best / median of 20 in ms")
rng = np.random.default_rng(1)
for label, names in (("benchmark library, 3 templates", H.TEMPLATE_ORDER), ("one template per marker, 16 templates", DS.library(16, size=4, seed=31))):
    frames = np.stack([H.synth_frame(cfg, i, names)[0] for i in range(N)])
    d = torch.from_numpy(frames).cuda()
    work = d.clone()
    det = oa.Detector(W, Hh, max_batch=N)
    det.set_templates([oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates(names)])
    det.set_camera(oa.Camera.from_buffer_copy(bytes(H.oracle_camera(W, Hh))))
    for t in range(len(names)):
        ov = rng.integers(0, 256, (256, 256, 4), dtype=np.uint8)
        ov[..., 3] = 255
        det.set_overlay(t, ov)
    dm = torch.zeros(N * det.max_markers * 184, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    det.enqueue_device(d.data_ptr(), W, Hh, N)
    det.results_to_device(dm.data_ptr(), dc.data_ptr())
    det.render(work.data_ptr(), W, Hh)
    markers, counts = det.collect()
    torch.cuda.synchronize()
    covered = float((work != d).any(dim=3).float().mean())
    stream = torch.cuda.current_stream().cuda_stream
    t_render = best(lambda: det.render_records(work.data_ptr(), W, Hh, N, dm.data_ptr(), dc.data_ptr(), stream=stream))
    t_copy = best(lambda: work.copy_(d))
    say(f"{label}: {counts.mean():.1f} records per frame, {100 * covered:.1f} % of the pixels drawn")
    say(f"  render (setup + draw kernels): {t_render[0]:.3f} / {t_render[1]:.3f} ms = {N / t_render[0] * 1e3:.0f} frames/s")
    say(f"  device copy of the frames:     {t_copy[0]:.3f} / {t_copy[1]:.3f} ms = {2 * N * W * Hh * 3 / t_copy[0] / 1e6:.0f} GB/s read + write")
    del det, d, work
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

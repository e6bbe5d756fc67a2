#!/usr/bin/env python3
"""Rates per input format (include/ocvar_hip.h: OCVAR_FMT_*) at 1920x1080, 16 markers, three templates, 256 distinct frames
resident on the device:
  isolated binarise_frames_kernel time per 2048-frame launch (stage_ms[0] of one context alone on the GPU, best of 3),
  the pipe's frames/s at the bench schedule (ocvar_hip_pipe_detect_device: 5 contexts, gate 2, 1638-frame chunks),
  ocvar_hip_detect_host frames/s from pageable and from caller-pinned memory, with and without grey_in_place.
One JSON line per format.    python tools/input_format_rate.py [formats, default bgr,rgb,bgra,rgba,gray]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import helpers as H
import opencv_ar_amd as oa

fmts = sys.argv[1].split(",") if len(sys.argv) > 1 else ["bgr", "rgb", "bgra", "rgba", "gray"]
B, UNIQ, N_PIPE, N_HOST = 2048, 256, 8192, 256
cfg = H.synth_config(3)
W, Hh = cfg.width, cfg.height
base = np.stack([H.synth_frame(cfg, i)[0] for i in range(UNIQ)])
tpls = oa.load_templates([os.path.join(oa.TEMPLATE_DIR, n + ".png") for n in H.TEMPLATE_ORDER])
cam = oa.default_camera(W, Hh)
rng = np.random.default_rng(0)
alpha = rng.integers(0, 256, (Hh, W, 1), dtype=np.uint8)


def in_format(fmt):
    if fmt == "gray":
        return np.ascontiguousarray(base[..., 0])
    src = base[..., ::-1] if fmt in ("rgb", "rgba") else base
    if fmt in ("bgra", "rgba"):
        src = np.concatenate([src, np.broadcast_to(alpha, (UNIQ, Hh, W, 1))], 3)
    return np.ascontiguousarray(src)


for fmt in fmts:
    frames = in_format(fmt)
    d_uniq = torch.from_numpy(frames).cuda()
    d = d_uniq[torch.arange(N_PIPE, device="cuda") % UNIQ].contiguous()
    torch.cuda.synchronize()
    out = {"format": fmt, "width": W, "height": Hh, "bytes_per_pixel": frames[0].nbytes // (W * Hh), "library": oa.build_info()}

    det = oa.Detector(W, Hh, max_batch=B)
    det.set_templates(tpls)
    det.set_camera(cam)
    det.set_input_format(fmt)
    ms = []
    for rep in range(4):
        det.enqueue_device(d.data_ptr(), W, Hh, B)
        _, c = det.collect(8)
        ms.append(float(det.stage_ms()[0]))
    out["binarise_frames_ms_per_2048"] = round(min(ms[1:]), 4)
    out["binarise_frames_fps_isolated"] = round(B / (min(ms[1:]) * 1e-3))
    out["markers_per_frame"] = round(float(c.mean()), 3)
    out["batch_ms_per_2048"] = round(float(det.stage_ms()[11]), 3)
    det.close()

    pipe = oa.Pipe(W, Hh, chunk_frames=1638, n_contexts=5, gate_width=2)
    pipe.set_templates(tpls)
    pipe.set_camera(cam)
    pipe.set_input_format(fmt)
    pipe.detect_device(d.data_ptr(), W, Hh, 4 * 1638, max_per_frame=8)
    best = 0.0
    for rep in range(3):
        t0 = time.perf_counter()
        pipe.detect_device(d.data_ptr(), W, Hh, N_PIPE, max_per_frame=8)
        best = max(best, N_PIPE / (time.perf_counter() - t0))
    out["pipe_fps_5ctx_gate2"] = round(best)
    pipe.close()
    del d, d_uniq
    torch.cuda.empty_cache()

    det = oa.Detector(W, Hh, max_batch=64)
    det.set_templates(tpls)
    det.set_camera(cam)
    det.set_input_format(fmt)
    host = frames[np.arange(N_HOST) % UNIQ]
    pinned = torch.empty(host.shape, dtype=torch.uint8, pin_memory=True).numpy()
    for label, buf in (("pageable", np.empty_like(host)), ("pinned", pinned)):
        for grey in (False, True):
            buf[:] = host
            det.detect_host(buf, grey_in_place=grey)   # (warm-up: staging buffers)
            buf[:] = host
            t0 = time.perf_counter()
            det.detect_host(buf, grey_in_place=grey)
            out[f"detect_host_fps_{label}{'_grey_in_place' if grey else ''}"] = round(N_HOST / (time.perf_counter() - t0))
    det.close()
    del pinned, host
    print(json.dumps(out), flush=True)

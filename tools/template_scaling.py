#!/usr/bin/env python3
"""frames/s and per-stage device time against the size of the template library.

The benchmark's geometry (BASELINE.json configs[2]: 1920x1080, 16 planted markers per frame) with single-size libraries of K
random 8x8 codes (K = 3, 16, 64, 256, 1024, 4096 by default); the synthetic generator plants markers from the library (frame i:
templates i .. i+15 mod K), so every frame decodes, matches and eliminates against the whole library.  Per K:
  pipe      frames/s of the streaming form (Pipe.submit / collect: CONTEXTS contexts of CHUNK frames, gate 2, as tools/pipe_rate.py)
  alone     one context, one CHUNK-frame batch alone on the GPU: stage_ms of order/crops, decode, dedupe+pose (mean of 3)
One JSON line per K and a summary line with each K's frames/s relative to the first.

    python tools/template_scaling.py [--ks 3,16,64,256,1024,4096] [--chunk 2048] [--contexts 4] [--chunks 48] [--unique 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import helpers as H  # noqa: E402
import opencv_ar_amd as oa  # noqa: E402


def library(k):
    rng = np.random.default_rng(k)
    names = []
    for i in range(k):
        name = f"scaling-{k}-{i}"
        H.register_template(name, rng.integers(0, 2, (8, 8)))
        names.append(name)
    return names, [oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates(names)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="3,16,64,256,1024,4096")
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--chunks", type=int, default=48)
    ap.add_argument("--unique", type=int, default=64)
    a = ap.parse_args()
    cfg = H.synth_config(3)
    W, Hh = cfg.width, cfg.height
    cam = oa.default_camera(W, Hh)
    pipe = oa.Pipe(W, Hh, chunk_frames=a.chunk, n_contexts=a.contexts, gate_width=2)
    pipe.set_camera(cam)
    pipe.set_result_limit(8)
    det = oa.Detector(W, Hh, max_batch=a.chunk)
    det.set_camera(cam)
    stage = {n: i for i, n in enumerate(oa.STAGE_NAMES)}
    rows = []
    for k in [int(x) for x in a.ks.split(",")]:
        names, tpls = library(k)
        base = np.stack([H.synth_frame(cfg, i, names)[0] for i in range(a.unique)])
        d = torch.from_numpy(base).cuda().repeat((a.chunk + a.unique - 1) // a.unique, 1, 1, 1)[:a.chunk].contiguous()
        torch.cuda.synchronize()
        pipe.set_templates(tpls)
        det.set_templates(tpls)
        # one batch alone: the stage times
        st = np.zeros(12)
        for rep in range(4):
            m, c = det.detect_device(d.data_ptr(), W, Hh, a.chunk, max_per_frame=8)
            if rep:
                st += det.stage_ms() / 3
        # streaming, first chunks staggered (tools/pipe_rate.py)
        sizes = [a.chunk * (i + 1) // a.contexts if i < a.contexts else a.chunk for i in range(a.chunks)]
        best = 0.0
        for rep in range(2):
            t0 = time.perf_counter()
            sub = done = 0
            while done < a.chunks:
                while sub < a.chunks and pipe.submit(d.data_ptr(), W, Hh, sizes[sub], tag=sub):
                    sub += 1
                tag, _, _ = pipe.collect(a.chunk, 8)
                assert tag == done
                done += 1
            best = max(best, sum(sizes) / (time.perf_counter() - t0))
        row = {"K": k, "frames_per_s": round(best), "markers_per_frame": round(float(c.mean()), 2),
               "stage_ms_alone": {n: round(float(st[stage[n]]), 4) for n in ("order_crops", "decode", "dedupe_pose", "batch_total")}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"relative_frames_per_s": {r["K"]: round(r["frames_per_s"] / rows[0]["frames_per_s"], 3) for r in rows},
                      "chunk": a.chunk, "contexts": a.contexts, "chunks": a.chunks, "build": oa.build_info()}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""frames/s and per-stage device time of dense contexts (ocvar_hip_create_dense) against the number of markers per frame.

Synthetic upright 50 px markers of a library of distinct random 4x4 codes (tests/dense_synth.py), one template per marker, on a
grid of about 64 / 256 / 1024 / as many as fit markers per frame, at 1920x1080 and 3840x2160.  Per case one dense context
(max_quads 16384, max_markers 4096) detects a batch of BATCH frames (UNIQUE distinct ones tiled) REPS times; reported: the
mean frames/s of the timed batches, the mean stage_ms of order+crops, decode and dedupe+pose per frame, the oracle-free
marker and square counts of the batch's first frame.  A case that fails (OCVAR_E_CAPACITY) is recorded with its flags.  One JSON line per case to stdout and to profiles/dense_scaling.jsonl.

    python tools/dense_scaling.py [--batch 16] [--unique 4] [--reps 5]
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

import dense_synth as D  # noqa: E402
import opencv_ar_amd as oa  # noqa: E402

# (width, height, grid_x, grid_y): ~64, ~256, ~1024 and the densest grid of 50 px markers (80 px cells)
CASES = [(1920, 1080, 8, 8), (1920, 1080, 16, 16), (1920, 1080, 24, 13),
         (3840, 2160, 8, 8), (3840, 2160, 16, 16), (3840, 2160, 32, 32), (3840, 2160, 48, 27)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--unique", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_scaling.jsonl"))
    a = ap.parse_args()
    stage = {n: i for i, n in enumerate(oa.STAGE_NAMES)}
    names = D.library(48 * 27)
    tpls = None
    rows = []
    dets = {}
    for W, Hh, gx, gy in CASES:
        key = (W, Hh)
        if key not in dets:
            det = oa.Detector(W, Hh, max_batch=a.batch, max_quads=16384, max_markers=4096)
            if tpls is None:
                import helpers as H
                tpls = [oa.Template.from_buffer_copy(bytes(t)) for t in H.oracle_templates(names)]
            det.set_templates(tpls)
            det.set_camera(oa.default_camera(W, Hh))
            dets[key] = det
        det = dets[key]
        cfg = D.config(W, Hh, gx, gy)
        base = np.stack([D.frame(cfg, i, names) for i in range(a.unique)])
        d = torch.from_numpy(base).cuda().repeat((a.batch + a.unique - 1) // a.unique, 1, 1, 1)[:a.batch].contiguous()
        # (the tiling kernel runs on torch's stream, the detector on its own: the frames must be complete before it reads them)
        torch.cuda.synchronize()
        try:
            markers, counts = det.detect_device(d.data_ptr(), W, Hh, a.batch)   # warm-up
        except oa.OcvarError as e:   # a capacity failure is a result too: recorded, never hidden
            row = dict(width=W, height=Hh, grid=[gx, gy], batch=a.batch, error=str(e),
                       capacity_flags=int(oa.hip_lib().ocvar_hip_capacity_flags(det._ctx)))
            print(json.dumps(row), flush=True)
            rows.append(row)
            continue
        times, st = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            markers, counts = det.detect_device(d.data_ptr(), W, Hh, a.batch)
            times.append(time.perf_counter() - t0)
            st.append(det.stage_ms())
        st = np.mean(st, axis=0)
        _, nsq = det.find_squares(base[0][:, :, 0])
        row = dict(width=W, height=Hh, grid=[gx, gy], batch=a.batch, markers_per_frame=int(counts[0]), squares_per_frame=int(nsq),
                   frames_per_s=round(a.batch / float(np.mean(times)), 1),
                   order_crops_ms_per_frame=round(float(st[stage["order_crops"]]) / a.batch, 4),
                   decode_ms_per_frame=round(float(st[stage["decode"]]) / a.batch, 4),
                   dedupe_pose_ms_per_frame=round(float(st[stage["dedupe_pose"]]) / a.batch, 4),
                   batch_ms=round(float(st[stage["batch_total"]]), 3), build=oa.build_info())
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

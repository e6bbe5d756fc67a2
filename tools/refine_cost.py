#!/usr/bin/env python3
"""Cost of corner refinement (ocvar_hip_set_corner_refine) on the benchmark's schedule: config 3 frames through a Pipe of 5
contexts at gate width 2 in chunks of 1638 frames, streaming (submit / collect, the first chunks staggered as bench.py does),
with refinement off and at 5 / 30 / 0.1 in alternating runs of one process.  Prints frames/s of each run and the median of each
setting.   python tools/refine_cost.py [chunks per run] [runs per setting] [half_win]"""
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

n_chunks = int(sys.argv[1]) if len(sys.argv) > 1 else 24
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
half_win = int(sys.argv[3]) if len(sys.argv) > 3 else 5
chunk, nctx, gate, uniq = 1638, 5, 2, 256
cfg = H.synth_config(3)
W, Hh = cfg.width, cfg.height
base = np.stack([H.synth_frame(cfg, i)[0] for i in range(uniq)])
per = 4
d = torch.from_numpy(base).cuda().repeat((per * chunk + uniq - 1) // uniq, 1, 1, 1)[:per * chunk].contiguous()
torch.cuda.synchronize()
pipe = oa.Pipe(W, Hh, chunk_frames=chunk, n_contexts=nctx, gate_width=gate)
pipe.set_templates(oa.load_templates([os.path.join(oa.TEMPLATE_DIR, x + ".png") for x in H.TEMPLATE_ORDER]))
pipe.set_camera(oa.default_camera(W, Hh))
pipe.set_result_limit(8)


def run():
    sizes = [chunk * (i + 1) // nctx if i < nctx else chunk for i in range(n_chunks)]
    t0 = time.perf_counter()
    sub = done = 0
    markers = 0
    while done < n_chunks:
        while sub < n_chunks and pipe.submit(d.data_ptr() + (sub % per) * chunk * W * Hh * 3, W, Hh, sizes[sub], tag=sub):
            sub += 1
        tag, m, c = pipe.collect(chunk, 8)
        assert tag == done and len(c) == sizes[done]
        markers += int(c.sum())
        done += 1
    return sum(sizes) / (time.perf_counter() - t0), markers / sum(sizes)


rates = {0: [], half_win: []}
run()   # warm-up
for r in range(runs):
    for w in (0, half_win):
        pipe.set_corner_refine(w, 30, 0.1)
        fps, mpf = run()
        rates[w].append(fps)
        print(f"run {r}, refine {'off' if w == 0 else f'{w} / 30 / 0.1'}: {fps:.0f} frames/s ({mpf:.2f} markers per frame)", flush=True)
off, on = np.median(rates[0]), np.median(rates[half_win])
print(f"median: off {off:.0f} frames/s, on {on:.0f} frames/s ({100 * (on - off) / off:+.2f} %)")

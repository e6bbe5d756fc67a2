#!/usr/bin/env python3
"""Compare the outputs of a timed bench.py run (bench.py --dump-outputs DIR) with the oracle, frame by frame.

bench.py tiles `--unique` distinct synthetic frames over its batch (frame f of the batch is distinct frame f % unique, distinct
frame i being H.synth_frame(cfg, S.frame_of(rank, world, i), names)).  This rebuilds those frames, runs the oracle once per
distinct frame and checks every dumped frame's full marker count and its marker records (the first min(count, records kept)
of them) with the bars of tests/test_gpu_parity.py: ids, score, aspect ratio exact, square within 0.5 px, pose within 1e-4.
CPU only; exit 1 on the first mismatch.

    python tools/check_bench_dump.py DIR [--config 3] [--unique 256] [--rank 0 --world 1]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import helpers as H  # noqa: E402
from opencv_ar_amd import MARKER_DTYPE  # noqa: E402
from opencv_ar_amd import sharding as S  # noqa: E402
from test_gpu_parity import OracleFrame, check_markers  # noqa: E402


def load_dump(dirname, suffix=""):
    """(frame indices, markers [n][k] MARKER_DTYPE, counts [n]) as bench.py's dump_outputs wrote them"""
    def arr(name):
        return np.load(os.path.join(dirname, f"{name}{suffix}.npy"))
    idx = arr("frame_index").astype(np.int64)
    counts = arr("counts").astype(np.int32)
    k = arr("templateId").shape[1]
    markers = np.zeros((len(idx), k), MARKER_DTYPE)
    for name in MARKER_DTYPE.names:
        markers[name] = arr(name)
    return idx, markers, counts


def check_dump(dirname, config=3, unique=256, rank=0, world=1):
    """returns (frames checked, markers checked); raises AssertionError naming the frame and record on a mismatch"""
    idx, markers, counts = load_dump(dirname, f"_rank{rank}" if world > 1 else "")
    cfg = H.synth_config(config)
    names = ["2x2-01"] if config in (1, 2) else None
    tpls, cam = H.oracle_templates(names), H.oracle_camera(cfg.width, cfg.height)
    need = sorted(set((idx % unique).tolist()))
    with ThreadPoolExecutor(min(32, os.cpu_count() or 1)) as ex:   # (generator and oracle are C; ctypes releases the GIL)
        refs = dict(zip(need, ex.map(lambda i: OracleFrame(H.synth_frame(cfg, S.frame_of(rank, world, i), names)[0], tpls, cam,
                                                           planes=False), need)))
    for row, f in enumerate(idx):
        check_markers(row, refs[int(f % unique)], markers, counts, where=f"batch frame {int(f)} (distinct frame {int(f % unique)})")
    return len(idx), int(sum(min(int(c), markers.shape[1]) for c in counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--unique", type=int, default=256)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--world", type=int, default=1)
    a = ap.parse_args()
    t0 = time.time()
    try:
        n, nm = check_dump(a.dir, a.config, a.unique, a.rank, a.world)
    except AssertionError as e:
        print(f"check_bench_dump: MISMATCH {e}")
        return 1
    print(f"check_bench_dump: {n} frames, {nm} marker records equal to the oracle (config {a.config}, {a.unique} distinct frames, "
          f"rank {a.rank} of {a.world}), {time.time() - t0:.1f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Time the rank counts of the classifier report (csrc/rank.hip) at the GTSRB test set's shape, 12 630 x 43.

    python tools/bench_recog.py [--n 12630] [--classes 43] [--reps 200]

Prints one JSON line: the device time of one cy_rank_counts call (both kernels; device events around `reps` back-to-back calls
after a warm-up), the wall time of metrics.recog_report from numpy inputs to the three numbers (upload, label sort, count,
read-back, fold), and the pair count the kernel works through.  Kernel-level times come from a run of this script under
`rocprofv3 --kernel-trace --stats` (kernels rank_prep_kernel / rank_count_kernel)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import metrics  # noqa: E402
from capsyolo_amd._lib import call, query  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=12630)
    ap.add_argument('--classes', type=int, default=43)
    ap.add_argument('--reps', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_recog needs a GPU')
    N, C = a.n, a.classes
    rng = np.random.default_rng(46)
    y = rng.integers(0, C, N).astype(np.int64)
    s = 0.7 * rng.random((N, C))
    s[np.arange(N), y] += 0.4 * (rng.random(N) < 0.7)
    s = (np.round(s * 64) / 64).astype(np.float32)
    p = types.SimpleNamespace(n_classes=C)

    st, lt = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    order = torch.sort(lt, stable=True)[1].to(torch.int32)
    ws = torch.empty(int(query('cy_rank_ws_ints', N, C)), dtype=torch.int32, device='cuda')
    out = torch.zeros(8 * N + 2, dtype=torch.int32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        call('cy_rank_counts', st.data_ptr(), lt.data_ptr(), order.data_ptr(), N, C, ws.data_ptr(), out.data_ptr(),
             out.data_ptr() + 32 * N, out.data_ptr() + 32 * N + 4, stream)

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    call_ms = e0.elapsed_time(e1) / a.reps

    report = metrics.recog_report(y, s, p)
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        report = metrics.recog_report(y, s, p)
        walls.append(time.perf_counter() - t0)
    n_cls = np.bincount(y, minlength=C).astype(np.float64)
    pairs = float(N) * N * C + float(N) * N + float(N) * N + float((n_cls ** 2).sum())
    print(json.dumps({'n': N, 'classes': C, 'reps': a.reps, 'rank_counts_call_ms': call_ms, 'recog_report_wall_ms': 1e3 * min(walls),
                      'pairs': pairs, 'pairs_per_s': pairs / (call_ms * 1e-3), 'report': {k: float(v) for k, v in report.items()}}))


if __name__ == '__main__':
    main()

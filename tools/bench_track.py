#!/usr/bin/env python
"""Time the tracking step (csrc/track.hip, `cy_track_update`: one launch of one workgroup) alone.

    python tools/bench_track.py [--reps 2000] [--rounds 5]

(K, T, C) = (16, 32, 43) is the streaming detector's default (16 box slots, 32 tracks, the 43 GTSRB classes); (16, 256, 43) and
(64, 64, 43) sit at the pair cap, K T = cy_track_max_pairs() = 4096.  The detections are min(K, T) / 2 boxes of 30 pixels that drift
by 2 pixels a frame, so after the first call every one of them is matched: the greedy assignment walks min(K, T) / 2 rounds, each
one barrier.  The same frame is fed again and again (the tracks then see a sign that stopped: still one match per box).  Per case:
`rounds` measurements of device events around `reps` back-to-back calls after a warm-up; the median and the spread (min, max) of the
per-call time are reported, and the live tracks at the end, so that the work is seen to be done.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import serve  # noqa: E402
from capsyolo_amd._lib import query  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_track needs a GPU')
    stream = torch.cuda.current_stream().cuda_stream
    pairs = query('cy_track_max_pairs')
    out = {'reps': a.reps, 'rounds': a.rounds, 'max_pairs': pairs, 'cases': []}
    for K, T, C in ((16, 32, 43), (16, pairs // 16, 43), (64, pairs // 64, 43)):
        rng = np.random.RandomState(3)
        n = min(K, T) // 2
        xy = np.zeros((K, 4))
        c = np.stack([40.0 + 50.0 * (np.arange(n) % 10), 40.0 + 50.0 * (np.arange(n) // 10)], axis=1)
        xy[:n] = np.concatenate([c - 15.0, c + 15.0], axis=1)
        rect = np.zeros((K, 4), np.int32)
        rect[:n] = (1, 2, 1, 2)
        d_cnt = torch.tensor([n], dtype=torch.int32).cuda()
        d_xy, d_rect = torch.from_numpy(xy).cuda(), torch.from_numpy(rect).cuda()
        d_conf = torch.from_numpy(rng.uniform(0.5, 1.0, K).astype(np.float32)).cuda()
        d_sc = torch.from_numpy(rng.uniform(0.0, 1.0, (K, C)).astype(np.float32)).cuda()
        trk = serve.SignTracker(C, K, max_tracks=T)

        def launch():
            trk.launch(d_cnt.data_ptr(), d_xy.data_ptr(), d_conf.data_ptr(), d_rect.data_ptr(), d_sc.data_ptr(), stream)

        launch()
        d_xy += 2.0                                                       # one step, so that the tracks carry a velocity
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / a.reps)
        tr = trk.fetch()
        if tr.live != n or tr.births or (tr.det < 0).any():
            raise SystemExit('K=%d T=%d: %d live tracks of %d boxes, %d births, %d unmatched' % (K, T, tr.live, n, tr.births, (tr.det < 0).sum()))
        out['cases'].append({'K': K, 'T': T, 'C': C, 'boxes': n, 'live': tr.live, 'call_us': float(np.median(us)),
                             'call_us_min': float(np.min(us)), 'call_us_max': float(np.max(us))})
    print(json.dumps(out))


if __name__ == '__main__':
    main()

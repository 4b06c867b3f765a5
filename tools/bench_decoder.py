#!/usr/bin/env python
"""Time the fused decoder kernel (csrc/decoder.hip, capsyolo_amd.interpret.decode_capsules) against the per-layer path
(models.Decoder.forward: about a dozen launches with every intermediate in HBM) at n = 176 (one interpretation sweep) and n = 4096.

    python tools/bench_decoder.py [--reps 100] [--warmup 20] [--out profiles/decoder_fused.json]

Same process, same closed-form weights, same input vectors.  Every repetition is one call bracketed by its own pair of device
events on the stream it runs on; the two paths alternate repetition by repetition, so both see the same machine; the figure is the
median of the repetitions after the warm-up.  A call's time includes the host's enqueue where the device waits for it, which at
n = 176 is what the per-layer path consists of: that is the time a user of either path waits.  Prints one JSON line (and writes
it to --out): per n the two medians in microseconds, their ratio, the 10th / 90th percentiles, and the largest difference between
the two outputs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import interpret, models  # noqa: E402
from helpers import closed_form_state, make_params, wave  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--sizes', type=int, nargs='+', default=[176, 4096])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_decoder needs a GPU')
    if a.reps < 50:
        raise SystemExit('bench_decoder: at least 50 repetitions')
    net = models.CapsuleNet(make_params(model='capsule', n_classes=43, device='cuda'))
    net.load_state_dict(closed_form_state(net))
    net.cuda().eval()
    result = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    with torch.no_grad():
        for n in a.sizes:
            t = torch.from_numpy(wave((n, 16), 0.3, amp=1.0, freq=0.913)).cuda()
            paths = {'fused': lambda: interpret.decode_capsules(net, t), 'per_layer': lambda: net.decoder(t)}
            diff = float((paths['fused']() - paths['per_layer']()).abs().max().item())
            times = {k: [] for k in paths}
            for r in range(a.warmup + a.reps):
                for k, fn in paths.items():
                    us = timed(fn)
                    if r >= a.warmup:
                        times[k].append(us)
            torch.cuda.synchronize()
            row = {'max_abs_diff': diff}
            for k, v in times.items():
                row[k + '_us'] = float(np.median(v))
                row[k + '_p10_p90_us'] = [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
            row['per_layer_over_fused'] = row['per_layer_us'] / row['fused_us']
            result['sizes'][str(n)] = row
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if result['sizes'].get('176', {}).get('per_layer_over_fused', 1.0) < 1.0:
        raise SystemExit('the fused launch is slower than the per-layer path at n = 176')


if __name__ == '__main__':
    main()

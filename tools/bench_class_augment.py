#!/usr/bin/env python
"""What the classifier feed costs CapsuleNet's training step (batch 64, 32 x 32 x 3, reconstruction loss on), measured through main.py's
own epoch loop (`main.train`: shuffle, batching, feeder, step, one loss read-back per step):

  device_feeder   today's path: utils.shuffle gathers the whole set on the host, DeviceFeeder stages every batch in pinned memory,
                  copies it and runs cy_center_u8 -- the baseline
  resident_0      class_augment.ClassAugmentSource with aug_max_shift = 0, aug_max_light = 0: the same numbers from the resident set
  resident_jit    the same with 4 / 0.05: the augmentation itself

each as the eager loop and with --graph, in one process on one device, the six variants alternating epoch by epoch, `--repeats` epochs
each after one warm-up epoch each.  The figure per epoch is wall time / steps in ms (every step ends in loss.item(), so the clock
stops on finished work); reported are the median over the repeats and their min / max as the spread.

    python tools/bench_class_augment.py [--n_set 39168] [--repeats 5] [--launches 200] [--out profiles/class_augment.json]

Also: DeviceFeeder.host_ms (where the host side of the baseline feed goes, per batch), and the kernel's own time: `--launches`
launches of cy_gather_jitter_u8 (no tables / both tables) and of cy_center_u8 on the same 64 samples, each bracketed by its own
pair of device events, the three alternating, after 50 warm-up rounds; median and p10 / p90 in microseconds, and the bytes a launch
moves.  Prints one JSON line and writes it to --out.  Nothing here is asserted by a test."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import capsyolo_amd  # noqa: E402,F401
import main as cy_main  # noqa: E402
from capsyolo_amd import _lib, class_augment, dp  # noqa: E402
from capsyolo_amd.input_pipeline import DeviceFeeder  # noqa: E402

BATCH = 64


def timed_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def kernel_times(x_u8, labels, launches):
    dev = 'cuda'
    n = len(x_u8)
    set_d, lab_d = torch.from_numpy(x_u8).to(dev), torch.from_numpy(labels).to(dev)
    shift, light = class_augment.jitter_tables(n, 0, 0)
    sh_d, li_d = torch.from_numpy(shift).to(dev), torch.from_numpy(light).to(dev)
    idx = np.random.default_rng(1).permutation(n)[:BATCH].astype(np.int32)
    idx_d = torch.from_numpy(idx).to(dev)
    gathered = torch.from_numpy(np.ascontiguousarray(x_u8[idx])).to(dev)
    out = torch.empty((BATCH, 3, 32, 32), dtype=torch.float32, device=dev)
    y = torch.empty(BATCH, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    gather = lambda a, b: _lib.call('cy_gather_jitter_u8', set_d.data_ptr(), lab_d.data_ptr(), n, 32, 32, a, b, idx_d.data_ptr(), BATCH,
                                    out.data_ptr(), y.data_ptr(), err.data_ptr(), s)
    paths = {'gather_no_tables': lambda: gather(None, None),
             'gather_jitter': lambda: gather(sh_d.data_ptr(), li_d.data_ptr()),
             'center_u8': lambda: _lib.call('cy_center_u8', gathered.data_ptr(), out.data_ptr(), BATCH, 32, 32, 3, 1, s)}
    times = {k: [] for k in paths}
    for r in range(50 + launches):
        for k, fn in paths.items():
            us = timed_us(fn)
            if r >= 50:
                times[k].append(us)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    res = {'launches': launches,
           'bytes_per_launch': {'read_u8': BATCH * 32 * 32 * 3, 'read_tables_and_labels': BATCH * (4 + 8 + 4 + 8),
                                'write_f32': BATCH * 3 * 32 * 32 * 4}}
    for k, v in times.items():
        res[k + '_us'] = float(np.median(v))
        res[k + '_p10_p90_us'] = [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_set', type=int, default=39168, help='samples (the GTSRB training set, 39 209, in whole batches of 64)')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_class_augment needs a GPU')
    if a.repeats < 5 or a.launches < 200 or a.n_set < BATCH or a.n_set % BATCH:
        raise SystemExit('bench_class_augment: at least 5 repeats and 200 launches, n_set a multiple of %d' % BATCH)
    rng = np.random.default_rng(0)
    x_u8 = rng.integers(0, 256, (a.n_set, 32, 32, 3), dtype=np.uint8)
    labels = rng.integers(0, 43, a.n_set).astype(np.int64)
    idx = np.arange(a.n_set)

    args = cy_main.parser.parse_args(['--model', 'capsule', '--batch_size', str(BATCH), '--no_metric'])
    feeders = []

    class RecordingFeeder(DeviceFeeder):
        def __init__(self, *p, **kw):
            DeviceFeeder.__init__(self, *p, **kw)
            feeders.append(self)
    cy_main.DeviceFeeder = RecordingFeeder

    sources = {'device_feeder': None,
               'resident_0': class_augment.ClassAugmentSource(x_u8, labels, 0, 0, 0.0),
               'resident_jit': class_augment.ClassAugmentSource(x_u8, labels, 0, 4, 0.05)}
    variants = {}
    for graph in (False, True):
        torch.manual_seed(0)
        params = cy_main.load_params(cy_main.config.model_dir['capsule'], args)
        params.rank, params.world, params.graph = 0, 1, graph
        model_cls, loss_fn, _, _ = cy_main.model_loss_predict['capsule']
        model = model_cls(params).to(device=params.device)
        opt = cy_main.Adam([p for p in model.parameters() if p.requires_grad], lr=args.lr)
        bucket = dp.GradBucket(model)
        for name, src in sources.items():
            variants[(name, 'graph' if graph else 'eager')] = (params, model, opt, loss_fn, bucket, src)

    def epoch(key):
        params, model, opt, loss_fn, bucket, src = variants[key]
        params.augment_source = src
        data = (idx, idx.copy()) if src is not None else (x_u8, labels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cy_main.train(data[0], data[1], model, opt, loss_fn, None, params, bucket, False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return 1e3 * dt / (a.n_set // BATCH)

    ms = {k: [] for k in variants}
    for r in range(1 + a.repeats):
        for k in variants:
            feeders[:] = []
            v = epoch(k)
            if r >= 1:
                ms[k].append(v)
                if k[0] == 'device_feeder':
                    h = feeders[-1].host_ms
                    ms.setdefault(('host_ms', k[1]), []).append({q: h[q] / h['batches'] for q in ('wait_slot', 'stage_copy', 'issue')})
    result = {'device': torch.cuda.get_device_name(0), 'model': 'capsule', 'batch': BATCH, 'n_set': a.n_set, 'steps_per_epoch': a.n_set // BATCH,
              'repeats': a.repeats, 'set_bytes': int(x_u8.nbytes), 'ms_per_step': {}, 'device_feeder_host_ms_per_batch': {}}
    for k, v in ms.items():
        if k[0] == 'host_ms':
            result['device_feeder_host_ms_per_batch'][k[1]] = {q: float(np.median([e[q] for e in v])) for q in v[0]}
        else:
            result['ms_per_step']['%s_%s' % k] = {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(e) for e in v]}
    result['kernel'] = kernel_times(x_u8, labels, a.launches)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

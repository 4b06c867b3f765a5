#!/usr/bin/env python
"""ConvNet on the project's kernels (params.json "cnn_kernels": "hip") beside the plain-torch ConvNet of the same tree, in one process
on one device, the variants alternating sample by sample:

  kernels   cy_linear_fwd (+ bias + ReLU), cy_linear_dgrad (masked), cy_linear_wgrad (+ db) at N = 128, K = 32768 and M = 16, 64, 1024
            rows, beside torch's F.linear + relu, dy @ W (+ mask), dy^T @ x (+ column sums).  A sample is `--burst` launches
            back to back between two device events, divided by the burst; W (16.8 MB) stays in the last-level cache between
            launches, for both sides alike.  Reported: median and p10 / p90 in microseconds, the shares the forward chose, and the
            bytes and FLOP a launch needs (from the shapes), so that a rate can be read off.
  step      forward + loss + backward + Adam at batch 64 (dropout 0): the HIP model eager and as a replayed graph (GraphedStep), the
            torch model eager with torch.optim.Adam.  A sample is `--steps` steps and one loss read-back; milliseconds per step.
  serve     the eval forward on 16 crops (the classifier of the streaming detector at max_boxes = 16) under no_grad; a sample is
            `--steps` forwards and a synchronise; microseconds per forward.

    python tools/bench_convnet.py [--samples 30] [--burst 10] [--steps 20] [--out profiles/bench_convnet.json]

Prints one JSON line and writes it to --out.  Nothing here is asserted by a test."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import _lib, loss_fns, models, optim  # noqa: E402
from capsyolo_amd.graph_step import GraphedStep  # noqa: E402

N, K = 128, 32768


def stats(v, scale=1.0):
    v = np.asarray(v, dtype=np.float64) * scale
    return {'median': float(np.median(v)), 'p10': float(np.percentile(v, 10)), 'p90': float(np.percentile(v, 90))}


def burst_us(fn, burst):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / burst


def alternate(paths, samples, warm, sample_fn):
    out = dict((k, []) for k in paths)
    for r in range(warm + samples):
        for k, fn in paths.items():
            v = sample_fn(fn)
            if r >= warm:
                out[k].append(v)
    return out


def kernel_times(M, samples, burst):
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(M)
    x = torch.relu(torch.randn(M, K, device=dev, generator=g))
    w = torch.randn(N, K, device=dev, generator=g) * 0.01
    b = torch.randn(N, device=dev, generator=g)
    dy = torch.randn(M, N, device=dev, generator=g)
    y, dx, dw, db = (torch.empty(s, device=dev) for s in ((M, N), (M, K), (N, K), (N,)))
    shares, slice_, nws = (_lib.query(q, M, N, K) for q in ('cy_linear_fwd_shares', 'cy_linear_fwd_slice', 'cy_linear_fwd_ws_floats'))
    ws = torch.empty(max(nws, 1), device=dev)
    s = torch.cuda.current_stream().cuda_stream
    paths = {
        'hip_fwd': lambda: _lib.call('cy_linear_fwd', x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, 1, ws.data_ptr(), s),
        'torch_fwd': lambda: torch.relu(F.linear(x, w, b)),
        'hip_dgrad': lambda: _lib.call('cy_linear_dgrad', dy.data_ptr(), w.data_ptr(), dx.data_ptr(), x.data_ptr(), M, N, K, s),
        'torch_dgrad': lambda: torch.mm(dy, w).mul_(x > 0),
        'hip_wgrad': lambda: _lib.call('cy_linear_wgrad', dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), M, N, K, s),
        'torch_wgrad': lambda: (torch.mm(dy.t(), x), dy.sum(0)),
    }
    t = alternate(paths, samples, 5, lambda fn: burst_us(fn, burst))
    res = {'M': M, 'N': N, 'K': K, 'fwd_shares': shares, 'fwd_slice': slice_, 'fwd_partial_bytes': 4 * nws,
           'flop': 2 * M * N * K,
           'bytes': {'fwd': 4 * (M * K + N * K + M * N) + 8 * nws, 'dgrad': 4 * (N * K + 2 * M * K + M * N), 'wgrad': 4 * (M * K + N * K + M * N)}}
    for k, v in t.items():
        res[k + '_us'] = stats(v)
    return res


def _params(kernels):
    return types.SimpleNamespace(n_classes=43, dropout=0.0, device='cuda', model='cnn', cnn_kernels=kernels)


def _net(kernels, state=None):
    p = _params(kernels)
    torch.manual_seed(0)
    net = models.ConvNet(p).cuda()
    if state is not None:
        net.load_state_dict(state)
    return net, p


def step_times(samples, steps, batch=64):
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(batch, 3, 32, 32, device='cuda', generator=g)
    y = torch.randint(0, 43, (batch,), device='cuda', generator=g)
    runs = {}
    for name, kernels, graph in (('hip_eager', 'hip', False), ('hip_graph', 'hip', True), ('torch_eager', 'torch', False)):
        net, p = _net(kernels)
        net.train()
        params = [q for q in net.parameters() if q.requires_grad]
        opt = optim.Adam(params, lr=1e-3) if kernels == 'hip' else torch.optim.Adam(params, lr=1e-3)
        fwd = lambda m, xb, yb, p=p: (lambda o: (o, loss_fns.cnn_loss(o, yb, p)))(m(xb))
        if graph:
            gs = GraphedStep(net, fwd, opt, (x, y))
            one = lambda gs=gs: gs(x, y)[1]
        else:
            def one(net=net, opt=opt, fwd=fwd):
                _, loss = fwd(net, x, y)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss
        runs[name] = one

    def sample(one):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = one()
        loss.item()
        return 1e3 * (time.perf_counter() - t0) / steps
    t = alternate(runs, samples, 2, sample)
    return dict({'batch': batch, 'steps_per_sample': steps}, **dict((k + '_ms', stats(v)) for k, v in t.items()))


def serve_times(samples, steps, crops=16):
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(crops, 3, 32, 32, device='cuda', generator=g)
    hip, _ = _net('hip')
    plain, _ = _net('torch', hip.state_dict())
    runs = {'hip': hip.eval(), 'torch': plain.eval()}

    def sample(net):
        with torch.no_grad():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = net(x)
            torch.cuda.synchronize()
        assert out.shape == (crops, 43)
        return 1e6 * (time.perf_counter() - t0) / steps
    t = alternate(runs, samples, 2, sample)
    with torch.no_grad():
        diff = float((runs['hip'](x) - runs['torch'](x)).abs().max())
    return dict({'crops': crops, 'forwards_per_sample': steps, 'max_abs_difference': diff}, **dict((k + '_us', stats(v)) for k, v in t.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--burst', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_convnet needs a GPU')
    if a.samples < 10 or a.burst < 1 or a.steps < 5:
        raise SystemExit('bench_convnet: at least 10 samples, a burst of 1 and 5 steps')
    result = {'device': torch.cuda.get_device_name(0), 'samples': a.samples, 'burst': a.burst,
              'kernels': [kernel_times(M, a.samples, a.burst) for M in (16, 64, 1024)],
              'step': step_times(a.samples, a.steps), 'serve': serve_times(a.samples, a.steps)}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

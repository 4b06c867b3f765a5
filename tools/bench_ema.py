#!/usr/bin/env python
"""What optim.Adam's moving average of the parameters costs per training step on an MI355X: step time with
ema_decay off and on (0.999) for
  capsule_eager   experiments/capsule, 32 x 32, batch 32, reconstruction on, eager loop
  capsule_graph   the same step captured in a HIP graph (graph_step.GraphedStep) and replayed
  darkcapsule     bench.py's headline shape: 416 x 416, n_grid 13, batch 32, fp32
Off and on run on two models with the same initial weights, in alternating timed windows (--rounds of --steps steps each after --warmup
steps); the line reports every window and the medians.  `adam_ms` is the optimizer alone: repeated step() calls on the last gradients
between two device events (one launch either way; with the average it moves 36 bytes per element instead of 28).

    python tools/bench_ema.py [--steps 20 --rounds 3 --warmup 5] [--only NAME]        -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EMA_DECAY = 0.999


def _window(step, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def _adam_alone(opt, n=50):
    """ms per opt.step() on the gradients the last training step left (the parameters move: this is a timing, nothing else)."""
    import torch
    for _ in range(5):
        opt.step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        opt.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _compare(make, args, graph=False):
    """make(ema) -> (eager step function, optimizer, GraphedStep factory or None)."""
    steps, opts = {}, {}
    for ema in (False, True):
        step, opt, graphed = make(ema)
        for _ in range(args.warmup):
            step()
        if graph:
            g = graphed()
            step = g.run
            for _ in range(args.warmup):
                step()
        steps[ema], opts[ema] = step, opt
    windows = {False: [], True: []}
    for _ in range(args.rounds):
        for ema in (False, True):
            windows[ema].append(round(_window(steps[ema], args.steps), 4))
    out = {'off_ms': windows[False], 'on_ms': windows[True],
           'off_median_ms': round(statistics.median(windows[False]), 4), 'on_median_ms': round(statistics.median(windows[True]), 4)}
    out['delta_ms'] = round(out['on_median_ms'] - out['off_median_ms'], 4)
    if not graph:
        out['adam_ms'] = {'off': round(_adam_alone(opts[False]), 4), 'on': round(_adam_alone(opts[True]), 4)}
    n = sum(p.numel() for p in opts[True].ema)
    out['averaged_elements'] = int(n)
    out['extra_bytes_per_step'] = int(8 * n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', default=None, choices=('capsule_eager', 'capsule_graph', 'darkcapsule'))
    args = ap.parse_args()
    import torch
    import capsyolo_amd  # noqa: F401
    from capsyolo_amd import loss_fns, models, optim, synth
    from capsyolo_amd.graph_step import GraphedStep
    if not torch.cuda.is_available():
        raise SystemExit('bench_ema.py measures on the GPU: none is visible')
    dev = torch.device('cuda:0')
    kw = dict(ema_decay=EMA_DECAY)

    def capsule(ema):
        p = types.SimpleNamespace(n_classes=43, dropout=0.0, recon=True, recon_coef=5e-4, device='cuda', model='capsule')
        torch.manual_seed(0)
        net = models.CapsuleNet(p).to(dev).train()
        opt = optim.Adam([q for q in net.parameters() if q.requires_grad], lr=1e-3, **(kw if ema else {}))
        x = torch.from_numpy(synth.images(32, 32)).permute(0, 3, 1, 2).contiguous().to(dev)
        y = torch.from_numpy(synth.gtsrb_labels(32, 43)).to(dev)

        def fwd(m, xb, yb):
            sc, rec = m(xb, yb, True)
            return sc, loss_fns.capsule_loss(sc, yb, p, xb, rec)

        def step():
            _, loss = fwd(net, x, y)
            opt.zero_grad()
            loss.backward()
            opt.step()

        def graphed():
            g = GraphedStep(net, fwd, opt, (x, y))
            g.run = lambda: g(x, y)
            return g
        return step, opt, graphed

    def darkcapsule(ema):
        H, g, B = 416, 13, 32
        p = types.SimpleNamespace(n_classes=43, n_grid=g, n_boxes=2, dropout=0.0, recon=False, recon_coef=5e-4, darknet_input=H,
                                  device='cuda', n_iter=3, model='darkcapsule', precision='fp32')
        torch.manual_seed(0)
        net = models.DarkCapsuleNet(p).to(dev).train()
        opt = optim.Adam([q for q in net.parameters() if q.requires_grad], lr=1e-3, **(kw if ema else {}))
        x = torch.from_numpy(synth.images(B, H)).permute(0, 3, 1, 2).contiguous().to(dev)
        y = torch.from_numpy(synth.gtsdb_labels(B, g, 43)).to(dev)

        def step():
            loss = loss_fns.darkcapsule_loss(net(x), y, p)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return step, opt, None

    res = {'options_on': kw, 'steps': args.steps, 'rounds': args.rounds, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}
    for name, make, graph in (('capsule_eager', capsule, False), ('capsule_graph', capsule, True), ('darkcapsule', darkcapsule, False)):
        if args.only in (None, name):
            res[name] = _compare(make, args, graph)
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Reproducer of an open finding: graph_step.GraphedStep around a PURE-TORCH model does not reliably follow the
eager run.  The model is two parameters behind elementwise operations and `mean`, whose gradients repeat to the bit, so a captured
and an eager run from the same start should agree bit for bit.  Seen on an MI355X: in some processes they do, in others the
parameters part from the second replay on (by up to 5e-2), or the loss tensor the replay returns holds other values while the
parameters stay right; with max_grad_norm the gradient norms part at the second replay.  It shows with ema_decay=None as with it.
The project's own models under GraphedStep have not shown it.  Cause not found.

    python tools/probe/graphed_step_torch_model.py        -> per run and step: losses, gradient statistics, largest parameter difference
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Elementwise(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        self.w = torch.nn.Parameter(torch.randn(70001, generator=g))
        self.b = torch.nn.Parameter(torch.randn(257, generator=g))

    def forward(self, x):
        return torch.tanh(x * self.w) + self.b.mean()


def run(ema, max_norm):
    from capsyolo_amd import optim
    from capsyolo_amd.graph_step import GraphedStep
    net_e, net_g = Elementwise().cuda(), Elementwise().cuda()
    g = torch.Generator().manual_seed(22)
    xs = [torch.randn((4, 70001), generator=g).cuda() for _ in range(6)]
    ys = [torch.randn((4, 70001), generator=g).cuda() for _ in range(6)]

    def fwd(m, x, y):
        out = m(x)
        return out, ((out - y) ** 2).mean()
    kw = dict(lr=1e-2, max_grad_norm=max_norm)
    if ema:
        kw.update(ema_decay=0.9, ema_warmup=True)
    opt_e, opt_g = optim.Adam(list(net_e.parameters()), **kw), optim.Adam(list(net_g.parameters()), **kw)
    step = GraphedStep(net_g, fwd, opt_g, (xs[0], ys[0]), warmup=3)
    print('ema %s max_grad_norm %s' % (ema, max_norm))
    for t, (x, y) in enumerate(zip(xs, ys), 1):
        _, loss = fwd(net_e, x, y)
        opt_e.zero_grad()
        loss.backward()
        opt_e.step()
        _, loss_g = step(x, y)
        torch.cuda.synchronize()
        diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(net_g.parameters(), net_e.parameters()))
        stats = (opt_e.grad_stats()['norm'], opt_g.grad_stats()['norm']) if max_norm is not None else ()
        print('  step %d: loss eager %.9g captured %.9g, norms %s, largest parameter difference %.3g'
              % (t, float(loss.detach()), float(loss_g.detach()), stats, diff))


def main():
    import capsyolo_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit('this probe runs on the GPU: none is visible')
    for ema, max_norm in ((False, 1e-3), (False, None), (True, 1e-3), (True, None)):
        run(ema, max_norm)


if __name__ == '__main__':
    main()

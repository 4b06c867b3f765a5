#!/usr/bin/env python
"""The image gradient and the attacks built on it (capsyolo_amd.attack), timed on CapsuleNet and on the HIP ConvNet in eval mode at one
batch, in one process on one device:

  input_gradient   one attack.input_gradient call (forward + loss + the input-gradient chain down to the image), milliseconds, and the
                   conv_image_grad launch inside it from ops.timer's device events, beside the kernel's own bounds: the bytes of dy
                   (and act) it must read, and the FLOP of its sum
  fgsm             one FGSM pass (that call plus the step kernel)
  pgd10            a 10-step PGD
  train_step       forward + loss + backward + Adam of the same model at the same batch (the step tools/bench_capsule.py and
                   tools/bench_convnet.py time), for the comparison DESIGN section 6r makes

A sample is `--reps` calls between two synchronisations; median, p10 and p90 over `--samples` samples after 3 warm-up samples.

    python tools/bench_attack.py [--batch 1024] [--samples 20] [--reps 3] [--out profiles/bench_attack.json]

Prints one JSON line and writes it to --out.  Nothing here is asserted by a test."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import attack, loss_fns, models, ops, optim  # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {'median': float(np.median(v)), 'p10': float(np.percentile(v, 10)), 'p90': float(np.percentile(v, 90))}


def timed(fn, samples, reps, warm=3):
    out = []
    for r in range(warm + samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append(1e3 * (time.perf_counter() - t0) / reps)
    return stats(out)


def bench_model(name, batch, samples, reps):
    if name == 'capsule':
        p = types.SimpleNamespace(n_classes=43, recon=False, recon_coef=5e-4, device='cuda', model='capsule')
        torch.manual_seed(0)
        net, loss_fn = models.CapsuleNet(p).cuda(), loss_fns.capsule_loss
        first = dict(Cout=256, k=9, pad=0, act=True)
    else:
        p = types.SimpleNamespace(n_classes=43, dropout=0.0, device='cuda', model='cnn', cnn_kernels='hip')
        torch.manual_seed(0)
        net, loss_fn = models.ConvNet(p).cuda(), loss_fns.cnn_loss
        first = dict(Cout=64, k=3, pad=1, act=True)
    g = torch.Generator(device='cuda').manual_seed(1)
    x = ((torch.randint(0, 256, (batch, 3, 32, 32), device='cuda', generator=g).float() - 128) / 128).contiguous()
    y = torch.randint(0, 43, (batch,), device='cuda', generator=g)
    eps = 2 * attack.GREY
    # the training step of the same model at the same batch
    net.train()
    opt = optim.Adam([q for q in net.parameters() if q.requires_grad], lr=1e-3)

    def step():
        loss = loss_fn(net(x), y, p)
        opt.zero_grad()
        loss.backward()
        opt.step()
    res = {'model': name, 'batch': batch, 'train_step_ms': timed(step, samples, reps)}
    net.eval()
    res['input_gradient_ms'] = timed(lambda: attack.input_gradient(net, x, y, p, loss_fn), samples, reps)
    res['fgsm_ms'] = timed(lambda: attack.fgsm(net, x, y, p, loss_fn, eps), samples, reps)
    res['pgd10_ms'] = timed(lambda: attack.pgd(net, x, y, p, loss_fn, eps, eps / 4, 10), max(samples // 2, 5), 1)
    # the launches of one input_gradient call, from device events
    ops.timer.reset()
    ops.timer.enabled = True
    try:
        for _ in range(10):
            attack.input_gradient(net, x, y, p, loss_fn)
        torch.cuda.synchronize()
        summ = ops.timer.summary()
    finally:
        ops.timer.enabled = False
        ops.timer.reset()
    res['launch_ms'] = dict((k, v[1]) for k, v in sorted(summ.items()))
    Ho = 32 + 2 * first['pad'] - first['k'] + 1
    plan = ops.image_grad_plan((batch, 3, 32, 32), first['Cout'], first['k'], 1, first['pad'])
    res['conv_image_grad'] = {
        'ms': [v[1] for k, v in summ.items() if k.startswith('conv_image_grad')][0],
        'blocks': plan.blocks, 'chunks': plan.chunks,
        'bytes_read': 4 * batch * Ho * Ho * first['Cout'] * (2 if first['act'] else 1),
        'bytes_written': 4 * batch * 3 * 32 * 32,
        # the sum as written (every tap of every image pixel, on or off the map) and the part that is on the map
        'flop_issued': 2 * batch * 32 * 32 * 3 * first['Cout'] * first['k'] ** 2,
        'flop_on_map': 2 * batch * Ho * Ho * 3 * first['Cout'] * first['k'] ** 2}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_attack needs a GPU')
    if a.samples < 5 or a.reps < 1 or a.batch < 1:
        raise SystemExit('bench_attack: at least 5 samples, 1 repetition and a batch of 1')
    result = {'device': torch.cuda.get_device_name(0), 'samples': a.samples, 'reps': a.reps,
              'models': [bench_model(m, a.batch, a.samples, a.reps) for m in ('capsule', 'cnn')]}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Generate tests/golden/interpret.npz by RUNNING THE REFERENCE (torch-CPU), like make_golden_recog.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_interpret.py

Needs the reference checkout (CAPSYOLO_REFERENCE).  The reference's CapsuleNet with helpers.closed_form_state is driven the way its
capsule_interpret.py drives it (conv1 -> primary_capsules -> traffic_sign_capsules -> gather of the labelled capsule -> for every
component v and offset c: `t[v] = t[v] + c`, decoder, `t[v] = t[v] - c`, in place, in float32), on helpers.synth_images(3, 32, 7)
with labels [3, 17, 42].  The fixture holds data only:

  recipe, labels, deltas (np.arange(11) * 0.05 - 0.25 as float32), caps [3,43,16] float32
  dig32_sums [3,16,11,2] float64, dig32_samples [3,16,11,32] float32: helpers.grad_digest of every float32 reconstruction of that
      loop -- its two sums and every 8th of its 256 strided samples (DIGEST_PICK; all 258 values of all 528 digests, twice, would be
      2 MB, the fixture has to stay under 300 KB)
  dig64_sums, dig64_minus_dig32: the same digests from the reference's modules in float64 on the CLEAN vectors float32(t[v]) +
      float32(c) (no in-place drift); the samples are stored as their difference to dig32_samples (<= 2e-7, so float32 holds it to
      1e-14)
  full_vi [8,2], full32 [8,3,32,32] float32: whole reconstructions of sample 0 at the corners and the centre of the (v, i) grid
  sqerr32 / sqerr64 [3]: sum((x - decoder(t))^2) of the three unperturbed reconstructions
  loop_to_clean64: max |float32 loop - clean float64| over every element of every reconstruction; drift: max |t after the loop - t|
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
from helpers import closed_form_state, grad_digest, make_params, synth_images  # noqa: E402

REF = os.environ.get('CAPSYOLO_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
import models as ref_models        # noqa: E402

LABELS = [3, 17, 42]
DIGEST_PICK = np.concatenate([[0, 1], np.arange(2, 258, 8)])      # of helpers.grad_digest's 258 values: the sums, every 8th sample
FULL_VI = [(0, 0), (0, 10), (15, 0), (15, 10), (7, 5), (8, 5), (0, 5), (15, 5)]

if __name__ == '__main__':
    p = make_params(n_classes=43, device='cpu', model='capsule')
    model = ref_models.CapsuleNet(p)
    model.load_state_dict(closed_form_state(model))
    model.eval()
    model64 = copy.deepcopy(model).double()
    x = synth_images(3, 32, 7)                                     # NCHW float32
    cc = np.arange(11) * 0.05 - 0.25                               # capsule_interpret.py:59 (float64, as there)
    deltas = cc.astype(np.float32)
    caps_all = np.zeros((3, 43, 16), dtype=np.float32)
    dig32 = np.zeros((3, 16, 11, len(DIGEST_PICK)))
    dig64 = np.zeros_like(dig32)
    full32 = np.zeros((len(FULL_VI), 3, 32, 32), dtype=np.float32)
    sqerr32, sqerr64 = np.zeros(3), np.zeros(3)
    loop_to_clean, drift = 0.0, 0.0
    with torch.no_grad():
        for b in range(3):
            xx = torch.from_numpy(x[b:b + 1])
            yy = torch.from_numpy(np.array(LABELS[b]).reshape(1,))
            h = F.relu(model.conv1(xx))
            h = model.primary_capsules(h)
            h = model.traffic_sign_capsules(h).squeeze()           # [43,16]
            caps_all[b] = h.numpy()
            t = torch.gather(h.unsqueeze(0), 1, yy.repeat(16, 1).t().unsqueeze(1)).squeeze()    # capsule_interpret.py:58
            t0 = t.clone()
            assert torch.equal(t0, h[LABELS[b]])
            sqerr32[b] = float(((xx - model.decoder(t0)) ** 2).sum())
            sqerr64[b] = float(((xx.double() - model64.decoder(t0.double())) ** 2).sum())
            for v in range(16):
                for i, c in enumerate(cc):
                    t[v] = t[v] + c
                    decoded = model.decoder(t)                     # [1,3,32,32]
                    t[v] = t[v] - c
                    clean = t0.clone()
                    clean[v] = clean[v] + torch.tensor(deltas[i])  # float32 + float32
                    decoded64 = model64.decoder(clean.double())
                    dig32[b, v, i] = grad_digest(decoded)[DIGEST_PICK]
                    dig64[b, v, i] = grad_digest(decoded64)[DIGEST_PICK]
                    loop_to_clean = max(loop_to_clean, float((decoded.double() - decoded64).abs().max()))
                    if b == 0 and (v, i) in FULL_VI:
                        full32[FULL_VI.index((v, i))] = decoded[0].numpy()
            drift = max(drift, float((t - t0).abs().max()))
    samples32 = dig32[..., 2:].astype(np.float32)
    assert np.array_equal(samples32.astype(np.float64), dig32[..., 2:])          # samples of a float32 tensor
    arrays = {
        'recipe': np.array('reference CapsuleNet(n_classes=43) with helpers.closed_form_state, eval; x = helpers.synth_images(3, 32, 7); '
                           'labels [3, 17, 42]; the loop of capsule_interpret.py:58-68'),
        'labels': np.array(LABELS, dtype=np.int64), 'deltas': deltas, 'caps': caps_all, 'digest_pick': DIGEST_PICK.astype(np.int64),
        'dig32_sums': dig32[..., :2], 'dig32_samples': samples32,
        'dig64_sums': dig64[..., :2], 'dig64_minus_dig32': (dig64[..., 2:] - dig32[..., 2:]).astype(np.float32),
        'full_vi': np.array(FULL_VI, dtype=np.int64), 'full32': full32, 'sqerr32': sqerr32, 'sqerr64': sqerr64,
        'loop_to_clean64': np.float64(loop_to_clean), 'drift': np.float64(drift)}
    path = os.path.join(HERE, 'interpret.npz')
    np.savez_compressed(path, **arrays)
    print('caps max |.| %.4g; decoder output %.3f .. %.3f; loop vs clean fp64 %.3g; drift %.3g; sqerr %s'
          % (np.abs(caps_all).max(), full32.min(), full32.max(), loop_to_clean, drift, sqerr64))
    print('interpret.npz %.1f KB' % (os.path.getsize(path) / 1024.0))

#!/usr/bin/env python
"""Generate tests/golden/classaug.npz by RUNNING THE REFERENCE's utils.augmentation (utils.py:126-143), like make_golden_builddata.py.

    CAPSYOLO_REFERENCE=<checkout> MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_classaug.py

Needs the reference checkout (CAPSYOLO_REFERENCE) and matplotlib at generation time only.  The fixture holds data only: a centred
float64 batch x [4, 8, 8, 3] whose every value is (k - 128) / 128 for a byte k, the lightness increase the function drew, and what it
returned.  The function throws its shift away and returns the HSV round trip of the unshifted x on the 0..1 scale,
so the one thing it pins is the lightness arithmetic: out = hsv_to_rgb(rgb_to_hsv((x + 1) / 2) + (0, 0, d)).  The drawn d is
recovered by re-seeding np.random and replaying the function's draws in its order: randint(-4, 5, size=2), then rand().
"""
import os
import sys

os.environ.setdefault('MPLBACKEND', 'Agg')
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('CAPSYOLO_REFERENCE')
if not REF:
    raise SystemExit('set CAPSYOLO_REFERENCE to a checkout of the reference project')
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
import utils as ref_utils          # noqa: E402

SEED, MAX_SHIFT, MAX_LIGHT = 31, 4, 0.05      # seed 31 draws the shift (-2, 3) and d = 0.0479


def batch():
    k = np.random.default_rng(5).integers(0, 256, (4, 8, 8, 3)).astype(np.float64)
    k[0, 0, 0] = [0, 0, 0]                                             # black: saturation 0, becomes the grey 256 d
    k[0, 0, 1] = [255, 255, 255]
    k[0, 0, 2] = [128, 128, 128]                                       # grey: the centred zero
    k[0, 0, 3] = [0, 200, 17]                                          # one zero channel: it stays zero
    k[0, 0, 4] = [31, 0, 255]
    k[0, 0, 5] = [9, 254, 0]
    k[0, 0, 6] = [1, 1, 1]
    k[0, 0, 7] = [77, 77, 3]                                           # two channels share the maximum
    return k


if __name__ == '__main__':
    k = batch()
    x = (k - 128.0) / 128.0                                            # float64, every value exact
    np.random.seed(SEED)
    out = ref_utils.augmentation(x, 'capsule', MAX_SHIFT, MAX_LIGHT)
    np.random.seed(SEED)
    shift = np.random.randint(-MAX_SHIFT, MAX_SHIFT + 1, size=2)
    d = np.random.rand() * MAX_LIGHT
    assert out.shape == x.shape and out.dtype == np.float64 and 0 < d < MAX_LIGHT
    path = os.path.join(HERE, 'classaug.npz')
    np.savez_compressed(path, x=x, light=np.float64(d), shift_drawn=shift.astype(np.int64), out=np.asarray(out, dtype=np.float64),
                        seed=np.int64(SEED), max_light=np.float64(MAX_LIGHT))
    print('classaug.npz %.1f KB  d = %.17g  shift drawn (and thrown away) %s  out in [%.4f, %.4f] %s'
          % (os.path.getsize(path) / 1024.0, d, shift.tolist(), out.min(), out.max(), out.dtype))

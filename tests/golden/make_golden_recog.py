#!/usr/bin/env python
"""Generate tests/golden/recog.npz by RUNNING THE REFERENCE (numpy + sklearn), like make_golden_pipeline.py.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_recog.py

Needs the reference checkout (CAPSYOLO_REFERENCE) and scikit-learn.  The fixture holds data only: per case the recipe (a
string), the labels y, the float32 scores y_hat and what the reference's own metrics.recog_auc / recog_pr / recog_acc returned
for them; for the cases in which every class has positives and negatives also the per-class values of the sklearn calls the
reference makes per class and then drops (metrics.py:20-22, 61-65).
"""
import os
import sys
from types import SimpleNamespace

os.environ.setdefault('MPLBACKEND', 'Agg')
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('CAPSYOLO_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
import matplotlib.pyplot as plt    # noqa: E402
import metrics as ref_metrics      # noqa: E402
from sklearn.metrics import auc, average_precision_score, roc_curve   # noqa: E402


def labels(rng, n, C, cover):
    """cover: every class at least once (so that the per-class values exist)"""
    y = rng.integers(0, C, n)
    if cover:
        y[:C] = np.arange(C)
        rng.shuffle(y)
    return y.astype(np.int64)


def scored(rng, y, C, noise, lift):
    """scores in (0, 1) like capsule lengths: uniform noise, the labelled class lifted in about 70 % of the rows"""
    s = noise * rng.random((len(y), C))
    good = rng.random(len(y)) < 0.7
    s[np.arange(len(y)), y] += lift * good
    return s


def cases():
    out = []
    rng = np.random.default_rng(11)
    y = labels(rng, 97, 5, True)
    out.append(('ties', 'seed 11: 97 x 5, scores quantised to eighths (many ties)', y,
                np.round(scored(rng, y, 5, 0.8, 0.4) * 8) / 8, True))
    rng = np.random.default_rng(12)
    y = labels(rng, 333, 43, True)
    out.append(('mid', 'seed 12: 333 x 43, every class present', y, scored(rng, y, 43, 0.6, 0.5), True))
    rng = np.random.default_rng(13)
    y = labels(rng, 320, 43, False)
    out.append(('dense', 'seed 13: 320 x 43 (a multiple of 64 rows), scores quantised to 1/64 like the full-size test', y,
                np.round(scored(rng, y, 43, 0.7, 0.4) * 64) / 64, False))
    rng = np.random.default_rng(14)
    y = labels(rng, 64, 7, True)
    out.append(('equal', 'seed 14: 64 x 7, all scores equal', y, np.full((64, 7), 0.25), True))
    rng = np.random.default_rng(15)
    y = labels(rng, 120, 6, True)
    s = np.where(rng.random((120, 6)) < 0.5, 0.0, np.round(scored(rng, y, 6, 1.0, 0.5) * 4) / 4 - 0.5)
    s = s.astype(np.float32)
    zeros = np.flatnonzero(s.ravel() == 0)
    s.ravel()[rng.choice(zeros, 60, replace=False)] = -0.0
    assert np.signbit(s[s == 0]).sum() == 60 and (~np.signbit(s[s == 0])).sum() > 60
    out.append(('zeros', 'seed 15: 120 x 6, 60 negative zeros among positive zeros, values of both signs in quarters', y, s, True))
    rng = np.random.default_rng(16)
    y = labels(rng, 150, 43, False)
    s = 3.0 * rng.standard_normal((150, 43)) - 2.0
    s[np.arange(150), y] += 4.0 * (rng.random(150) < 0.7)
    out.append(('logits', 'seed 16: 150 x 43 ConvNet-like logits, mostly negative', y, s, False))
    return out


if __name__ == '__main__':
    arrays = {}
    for tag, recipe, y, s, per_class in cases():
        s = np.ascontiguousarray(s, dtype=np.float32)
        C = s.shape[1]
        p = SimpleNamespace(n_classes=C, model='capsule')
        r_auc = float(ref_metrics.recog_auc(y, s, p))
        r_pr = float(ref_metrics.recog_pr(y, s, p))
        r_acc = float(ref_metrics.recog_acc(y, s, p))
        plt.close('all')
        arrays.update({tag + '_recipe': np.array(recipe), tag + '_y': y, tag + '_y_hat': s, tag + '_auc': np.float64(r_auc),
                       tag + '_pr': np.float64(r_pr), tag + '_acc': np.float64(r_acc)})
        if per_class:
            onehot = np.eye(C)[y]
            assert (onehot.sum(0) > 0).all() and (onehot.sum(0) < len(y)).all()
            a, q = np.zeros(C), np.zeros(C)
            for i in range(C):
                fpr, tpr, _ = roc_curve(onehot[:, i], s[:, i])
                a[i] = auc(fpr, tpr)
                q[i] = average_precision_score(onehot[:, i], s[:, i])
            arrays.update({tag + '_auc_per_class': a, tag + '_pr_per_class': q})
        print('%-6s %3d x %2d  auc %.17g  pr %.17g  acc %.17g  per class: %s' % (tag, len(y), C, r_auc, r_pr, r_acc, per_class))
    arrays['cases'] = np.array([c[0] for c in cases()])
    path = os.path.join(HERE, 'recog.npz')
    np.savez_compressed(path, **arrays)
    print('recog.npz %.1f KB' % (os.path.getsize(path) / 1024.0))

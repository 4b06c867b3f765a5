"""numpy restatement of the rank counts behind recog_auc / recog_pr (csrc/rank.hip, capsyolo_amd.metrics.recog_counts) and of
their folds: sort + searchsorted on the host.  tests/test_recog_host.py pins it against tests/golden/recog.npz, which holds
what the reference's own recog_auc / recog_pr / recog_acc (sklearn) returned; the GPU tests compare the device against it
integer for integer."""
import numpy as np


def _ge_gt(pop, thr):
    """(number of elements of pop >= t, > t) for every t of thr; float compares, so -0.0 == +0.0."""
    pop = np.sort(np.asarray(pop))
    return len(pop) - np.searchsorted(pop, thr, side='left'), len(pop) - np.searchsorted(pop, thr, side='right')


def counts(y, s):
    """int64 [2][N][4] = (cnt_ge, cnt_gt, tp_ge, tp_gt) per row: micro, then per class.  s is compared as float32."""
    s = np.asarray(s).astype(np.float32)
    y = np.asarray(y).astype(np.int64)
    n = len(y)
    p = s[np.arange(n), y]
    out = np.zeros((2, n, 4), dtype=np.int64)
    out[0, :, 0], out[0, :, 1] = _ge_gt(s.ravel(), p)
    out[0, :, 2], out[0, :, 3] = _ge_gt(p, p)
    for c in np.unique(y):
        rows = np.flatnonzero(y == c)
        out[1, rows, 0], out[1, rows, 1] = _ge_gt(s[:, c], p[rows])
        out[1, rows, 2], out[1, rows, 3] = _ge_gt(p[rows], p[rows])
    return out


def correct(y, s):
    return int(np.sum(np.asarray(y) == np.argmax(np.asarray(s).astype(np.float32), axis=1)))


def auc(cnt, n_pos, n_neg):
    """ROC AUC (trapezoid over the distinct thresholds) of a population from the count rows of its positives."""
    if n_pos == 0 or n_neg == 0:
        return float('nan')
    neg_ge, neg_gt = cnt[:, 0] - cnt[:, 2], cnt[:, 1] - cnt[:, 3]
    num = int(np.sum(2 * (n_neg - neg_ge) + (neg_ge - neg_gt), dtype=np.int64))
    return num / (2 * n_pos * n_neg)


def ap(cnt, n_pos, n_neg):
    """Step-wise average precision; NaN without a positive or a negative (the per-class convention of the product)."""
    if n_pos == 0 or n_neg == 0:
        return float('nan')
    return float(np.sum(cnt[:, 2] / cnt[:, 0]) / n_pos)


def micro(y, s):
    """(recog_auc, recog_pr)"""
    s = np.asarray(s)
    n, C = s.shape
    cnt = counts(y, s)[0]
    return auc(cnt, n, n * (C - 1)), float(np.sum(cnt[:, 2] / cnt[:, 0]) / n)


def per_class(y, s):
    """([C] AUC, [C] AP)"""
    s = np.asarray(s)
    y = np.asarray(y).astype(np.int64)
    n, C = s.shape
    cnt = counts(y, s)[1]
    a, p = np.full(C, np.nan), np.full(C, np.nan)
    for c in range(C):
        rows = cnt[y == c]
        a[c], p[c] = auc(rows, len(rows), n - len(rows)), ap(rows, len(rows), n - len(rows))
    return a, p

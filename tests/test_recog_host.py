"""CPU tests of the classifier report: the numpy restatement of tests/rank_ref.py (the yardstick of tests/test_gpu_recog.py)
against what the reference's own recog_auc / recog_pr / recog_acc returned (tests/golden/recog.npz), and the C-ABI's new
symbols."""
import os
import re

import numpy as np
import pytest

from helpers import REPO, load_golden

import rank_ref as R
from capsyolo_amd import _lib

CASES = ['ties', 'mid', 'dense', 'equal', 'zeros', 'logits']
PER_CLASS = ['ties', 'mid', 'equal', 'zeros']
# Both sides are sums of at most N non-negative terms that total <= 1, in any order: a few ulps of 1.  Loose on purpose.
BOUND = 1e-12


@pytest.fixture(scope='module')
def gold():
    return load_golden('recog')


def test_fixture_holds_the_cases(gold):
    assert list(gold['cases']) == CASES
    assert all(gold[t + '_y_hat'].dtype == np.float32 and len(gold[t + '_y']) <= 333 for t in CASES)
    assert [t for t in CASES if t + '_auc_per_class' in gold] == PER_CLASS
    z = gold['zeros_y_hat']
    assert np.signbit(z[z == 0]).sum() == 60 and (~np.signbit(z[z == 0])).sum() > 60
    assert len(np.unique(gold['equal_y_hat'])) == 1 and (gold['logits_y_hat'] < 0).mean() > 0.5
    assert len(np.unique(gold['ties_y_hat'])) <= 13


@pytest.mark.parametrize('tag', CASES)
def test_restatement_reproduces_the_reference(gold, tag):
    y, s = gold[tag + '_y'], gold[tag + '_y_hat']
    auc, pr = R.micro(y, s)
    print('%s: auc off by %.3g, pr off by %.3g' % (tag, abs(auc - float(gold[tag + '_auc'])), abs(pr - float(gold[tag + '_pr']))))
    assert abs(auc - float(gold[tag + '_auc'])) <= BOUND
    assert abs(pr - float(gold[tag + '_pr'])) <= BOUND
    assert R.correct(y, s) / len(y) == float(gold[tag + '_acc'])


@pytest.mark.parametrize('tag', PER_CLASS)
def test_restatement_reproduces_the_per_class_values(gold, tag):
    a, p = R.per_class(gold[tag + '_y'], gold[tag + '_y_hat'])
    assert np.abs(a - gold[tag + '_auc_per_class']).max() <= BOUND
    assert np.abs(p - gold[tag + '_pr_per_class']).max() <= BOUND


def test_restatement_counts_by_brute_force(gold):
    """sort + searchsorted against the definition, all pairs, on the case with ties and the case with both zeros."""
    for tag in ('ties', 'zeros'):
        y, s = gold[tag + '_y'].astype(np.int64), gold[tag + '_y_hat']
        n, C = s.shape
        p = s[np.arange(n), y]
        pos = np.eye(C, dtype=bool)[y]
        want = np.zeros((2, n, 4), dtype=np.int64)
        for i in range(n):
            col, cpos = s[:, y[i]], y == y[i]
            want[0, i] = [(s >= p[i]).sum(), (s > p[i]).sum(), (s[pos] >= p[i]).sum(), (s[pos] > p[i]).sum()]
            want[1, i] = [(col >= p[i]).sum(), (col > p[i]).sum(), (col[cpos] >= p[i]).sum(), (col[cpos] > p[i]).sum()]
        assert np.array_equal(R.counts(y, s), want)


def test_per_class_values_are_nan_for_an_absent_or_a_universal_class():
    s = np.array([[0.1, 0.9, 0.3], [0.8, 0.2, 0.1], [0.3, 0.4, 0.2]], dtype=np.float32)
    a, p = R.per_class(np.array([1, 1, 0]), s)
    assert np.isnan(a[2]) and np.isnan(p[2]) and np.isfinite(a[:2]).all() and np.isfinite(p[:2]).all()
    a, p = R.per_class(np.array([1, 1, 1]), s)
    assert np.isnan(a).all() and np.isnan(p).all()


def test_cabi_declares_and_binds_the_rank_counts():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name in ('cy_rank_counts', 'cy_rank_ws_ints'):
        assert re.search(r'\b%s\s*\(' % name, header)
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(_lib._SIGS['cy_rank_counts']) == 10
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6


def test_rank_counts_refuses_what_does_not_fit_int32():
    """N * C >= 2^31: refused by the entry point's argument check, before any launch (the pointers are never followed)."""
    assert _lib.query('cy_rank_ws_ints', 12630, 43) == 12630 * 43 + 2 * 12630
    assert _lib.query('cy_rank_ws_ints', 1 << 16, 1 << 15) == 0 and _lib.query('cy_rank_ws_ints', 0, 43) == 0
    assert _lib.query('cy_rank_ws_ints', (1 << 16) - 1, 1 << 15) > 0
    with pytest.raises(_lib.HipExtensionError, match='int32'):
        _lib.call('cy_rank_counts', 16, 16, 16, 1 << 16, 1 << 15, 16, 16, 16, 16, None)
    with pytest.raises(_lib.HipExtensionError):
        _lib.call('cy_rank_counts', 16, 16, 16, 0, 43, 16, 16, 16, 16, None)
    with pytest.raises(_lib.HipExtensionError, match='null'):
        _lib.call('cy_rank_counts', 16, None, 16, 4, 43, 16, 16, 16, 16, None)

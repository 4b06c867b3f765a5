"""GPU tests of the classifier report (csrc/rank.hip behind capsyolo_amd.metrics.recog_counts / recog_auc / recog_pr, and
`main.py --mode predict --model capsule`).  The yardsticks are the numpy restatement of tests/rank_ref.py (pinned against the
reference by tests/test_recog_host.py) for the integer counts, and tests/golden/recog.npz, which holds what the reference's
own functions returned, for the values.

The kernel keeps 1024 thresholds per block (256 lanes x 4) and streams the population through LDS in tiles of 2048 elements;
the flat population is split into shares of whole tiles and the rows into chunks (at most one per 2048 rows)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, load_golden, make_params

import rank_ref as R
from capsyolo_amd import _lib, metrics, models, predict_fns, synth, utils

pytestmark = pytest.mark.gpu

FIXTURE = ['ties', 'mid', 'dense', 'equal', 'zeros', 'logits']
PER_CLASS = ['ties', 'mid', 'equal', 'zeros']
BOUND = 1e-12                    # as in test_recog_host.py: sums of <= N non-negative terms totalling <= 1, any order


@pytest.fixture(scope='module')
def gold():
    return load_golden('recog')


def _lifted(rng, n, C, q):
    """labels and scores quantised to 1/q (ties), the labelled class lifted in about 70 % of the rows"""
    y = rng.integers(0, C, n)
    s = 0.7 * rng.random((n, C))
    s[np.arange(n), y] += 0.4 * (rng.random(n) < 0.7)
    return y.astype(np.int64), (np.round(s * q) / q).astype(np.float32)


def _case(name):
    if name == 'n1':                                         # one row, two classes
        return np.array([1]), np.array([[0.3, 0.7]], dtype=np.float32)
    if name == 'odd':                                        # N is no multiple of the wavefront
        return _lifted(np.random.default_rng(41), 77, 5, 16)
    if name == 'blocks':                                     # 1025 rows > the 1024 thresholds of a block; 2050 elements > a tile of 2048
        return _lifted(np.random.default_rng(42), 1025, 2, 32)
    if name == 'chunks':                                     # 2049 rows: two row chunks, blocks whose thresholds span classes, a class over blocks
        return _lifted(np.random.default_rng(43), 2049, 3, 64)
    if name == 'all_equal':
        return np.random.default_rng(44).integers(0, 4, 130).astype(np.int64), np.full((130, 4), -1.5, dtype=np.float32)
    if name == 'signed_zeros':
        rng = np.random.default_rng(45)
        y = rng.integers(0, 5, 90).astype(np.int64)
        s = rng.choice(np.array([-0.0, 0.0, 0.0, -0.25, 0.25, 1e-42, -1e-42], dtype=np.float32), (90, 5))      # and two denormals
        return y, s
    if name == 'tied_max':                                   # the maximum tied left and right of the label: argmax takes the first
        s = np.array([[0.5, 0.9, 0.9, 0.9, 0.1], [0.5, 0.9, 0.9, 0.9, 0.1], [0.5, 0.9, 0.9, 0.9, 0.1], [0.9, 0.9, 0.2, 0.1, 0.9],
                      [0.9, 0.9, 0.2, 0.1, 0.9], [0.1, 0.1, 0.1, 0.1, 0.1]], dtype=np.float32)
        return np.array([2, 1, 3, 0, 4, 0]), s
    if name == 'full':                                       # the GTSRB test set's shape: the AUC numerator is about 1.3e10
        rng = np.random.default_rng(46)
        sizes = rng.integers(60, 750, 43).astype(np.float64)
        y = rng.choice(43, 12630, p=sizes / sizes.sum()).astype(np.int64)
        s = 0.7 * rng.random((12630, 43))
        s[np.arange(12630), y] += 0.4 * (rng.random(12630) < 0.7)
        return y, (np.round(s * 64) / 64).astype(np.float32)
    raise KeyError(name)


SEEDED = ['n1', 'odd', 'blocks', 'chunks', 'all_equal', 'signed_zeros', 'tied_max', 'full']


@pytest.mark.parametrize('name', FIXTURE + SEEDED)
def test_counts_equal_the_restatement_integer_for_integer(gold, name):
    y, s = (gold[name + '_y'], gold[name + '_y_hat']) if name in FIXTURE else _case(name)
    C = s.shape[1]
    counts, correct = metrics.recog_counts(y, s, C)
    assert counts.dtype == np.int64 and counts.shape == (2, len(y), 4)
    assert np.array_equal(counts, R.counts(y, s))
    assert correct == int(np.sum(y == np.argmax(s, axis=1)))
    p = make_params(n_classes=C)
    assert correct / len(y) == metrics.recog_acc(y, s, p)
    if C > 1:
        auc, pr = R.micro(y, s)
        got_auc, got_pr = metrics.recog_auc(y, s, p), metrics.recog_pr(y, s, p)
        print('%s: auc %.17g pr %.17g' % (name, got_auc, got_pr))
        assert abs(got_auc - auc) <= BOUND and abs(got_pr - pr) <= BOUND
    if name == 'tied_max':
        assert correct == 3                                  # rows 1, 3 and 5
    if name == 'full':
        cnt = counts[0]
        assert int(np.sum(2 * (len(y) * (C - 1) - (cnt[:, 0] - cnt[:, 2])), dtype=np.int64)) > 2 ** 32      # what an int32 fold loses


@pytest.mark.parametrize('tag', FIXTURE)
def test_values_against_the_reference(gold, tag):
    y, s = gold[tag + '_y'], gold[tag + '_y_hat']
    p = make_params(n_classes=s.shape[1])
    auc, pr = metrics.recog_auc(y, s, p, save=True, save_dir='/nonexistent'), metrics.recog_pr(y, s, p, show=False, save=False)
    print('%s: auc off by %.3g, pr off by %.3g' % (tag, abs(auc - float(gold[tag + '_auc'])), abs(pr - float(gold[tag + '_pr']))))
    assert abs(auc - float(gold[tag + '_auc'])) <= BOUND and abs(pr - float(gold[tag + '_pr'])) <= BOUND
    _, correct = metrics.recog_counts(y, s, s.shape[1])
    assert correct / len(y) == metrics.recog_acc(y, s, p) == float(gold[tag + '_acc'])
    report = metrics.recog_report(y, s, p)
    assert list(report) == ['recog_pr', 'recog_acc', 'recog_auc']
    assert report == {'recog_pr': pr, 'recog_acc': correct / len(y), 'recog_auc': auc}
    if tag in PER_CLASS:
        a, q = metrics.recog_auc_per_class(y, s, s.shape[1]), metrics.recog_pr_per_class(y, s, s.shape[1])
        assert a.shape == q.shape == (s.shape[1],)
        assert np.abs(a - gold[tag + '_auc_per_class']).max() <= BOUND and np.abs(q - gold[tag + '_pr_per_class']).max() <= BOUND


def test_per_class_values_of_an_absent_class_are_nan(gold):
    y, s = gold['dense_y'], gold['dense_y_hat']              # 320 rows over 43 classes; remove one class
    y = np.where(y == 7, 8, y)
    a, q = metrics.recog_auc_per_class(y, s, 43), metrics.recog_pr_per_class(y, s, 43)
    ra, rq = R.per_class(y, s)
    assert np.isnan(a[7]) and np.isnan(q[7]) and np.isfinite(np.delete(a, 7)).all()
    assert np.array_equal(a, ra, equal_nan=True) and np.array_equal(q, rq, equal_nan=True)


def test_input_forms_permutation_and_determinism(gold):
    y, s = gold['mid_y'], gold['mid_y_hat']
    base, correct = metrics.recog_counts(y, s, 43)
    again, correct2 = metrics.recog_counts(y, s, 43)
    assert np.array_equal(base, again) and correct == correct2                                   # two calls: identical bits
    dev, correct3 = metrics.recog_counts(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), 43)
    assert np.array_equal(base, dev) and correct == correct3                                     # device tensors
    p = make_params(n_classes=43)
    assert metrics.recog_auc(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), p) == metrics.recog_auc(y, s, p)
    assert metrics.recog_pr(y.astype(np.int32), s.astype(np.float64), p) == metrics.recog_pr(y, s, p)     # converted to float32 first
    perm = np.random.default_rng(9).permutation(len(y))
    moved, correct4 = metrics.recog_counts(y[perm], s[perm], 43)
    assert np.array_equal(moved, base[:, perm]) and correct4 == correct                          # rows move with their row, nothing else
    # float64 scores that differ only beyond float32 are ties
    wide = s.astype(np.float64) + 1e-12 * np.random.default_rng(10).random(s.shape)
    assert np.array_equal(metrics.recog_counts(y, wide, 43)[0], R.counts(y, wide.astype(np.float32)))


def test_bad_inputs_raise_and_nothing_faults(gold):
    y, s = gold['ties_y'].copy(), gold['ties_y_hat'].copy()
    for bad in (np.nan, np.inf, -np.inf):
        t = s.copy()
        t[13, 2] = bad
        with pytest.raises(ValueError, match='non-finite'):
            metrics.recog_counts(y, t, 5)
    for label in (5, -1, 2 ** 40):
        z = y.copy()
        z[20] = label
        with pytest.raises(ValueError):
            metrics.recog_auc(z, s, make_params(n_classes=5))
    with pytest.raises(ValueError):
        metrics.recog_counts(np.zeros(0, dtype=np.int64), np.zeros((0, 5), dtype=np.float32), 5)
    with pytest.raises(ValueError):
        metrics.recog_counts(y, s, 6)                        # the scores have 5 columns
    with pytest.raises(ValueError):
        metrics.recog_counts(y[:-1], s, 5)
    with pytest.raises(ValueError):
        metrics.recog_counts(y.astype(np.float64), s, 5)
    # one entry-point call per count, and the device is still in order: the good input gives the good answer
    _lib.TRACE = []
    try:
        counts, _ = metrics.recog_counts(y, s, 5)
        assert _lib.TRACE == ['cy_rank_counts']
    finally:
        _lib.TRACE = None
    assert np.array_equal(counts, R.counts(y, s))


def test_class_scores_device_and_main_predict_mode(tmp_path):
    cp = make_params(model='capsule', n_classes=43, device='cuda', batch_size=16)
    torch.manual_seed(3)
    cdir = str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.CapsuleNet(cp).state_dict()}, False, cdir)
    json.dump(dict(batch_size=16, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_predict_class', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(['--mode', 'predict', '--model', 'capsule', '--synthetic', '40', '--model_dir', cdir, '--restore', 'last'])
    text = open(os.path.join(cdir, 'metric_output.txt')).read()
    fields = dict(f.split(':') for f in text.split(', ') if f)
    assert list(fields) == ['recog_pr', 'recog_acc', 'recog_auc'] == list(out)
    for k, v in fields.items():
        assert np.isfinite(float(v)) and float(v) == float(out[k]) and 0.0 <= float(v) <= 1.0
    # the same numbers from the metrics called on class_pred's scores for the same data
    x, y = synth.images(40, 32), synth.gtsrb_labels(40, 43)
    caps = models.CapsuleNet(cp).cuda()
    scores, classes = predict_fns.class_pred(x, caps, cdir, cp, 'last', batch_size=16)
    assert scores.shape == (40, 43) and scores.dtype == np.float32
    assert out == {'recog_pr': metrics.recog_pr(y, scores, cp), 'recog_acc': metrics.recog_acc(y, scores, cp),
                   'recog_auc': metrics.recog_auc(y, scores, cp)}
    assert out['recog_acc'] == np.sum(y == classes) / 40
    auc, pr = R.micro(y, scores)
    assert abs(out['recog_auc'] - auc) <= BOUND and abs(out['recog_pr'] - pr) <= BOUND
    dev = predict_fns.class_scores_device(x, caps, cp, batch_size=16)
    assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy(), scores)      # bit for bit
    with pytest.raises(SystemExit):                          # no --restore
        m.main(['--mode', 'predict', '--model', 'capsule', '--synthetic', '40', '--model_dir', cdir])

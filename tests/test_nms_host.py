"""CPU tests of the suppression step (csrc/nms.hip, utils.nms_boxes_device / nms_y_hat_device, the nms arguments of predict_fns,
serve.SignDetector and main.py): the exports, the refusals that come before any device work, the known answers and the prefix
consistency of the numpy restatement tests/nms_ref.py, and the argument checks."""
import importlib.util
import os
import re

import numpy as np
import pytest

from helpers import REPO

import nms_ref as R
from capsyolo_amd import _lib, serve

ARGS = ('count_in', 'box_img', 'box_xy', 'conf', 'cls', 'n_cap', 'n_images', 'iou_th', 'class_aware', 'per_image', 'max_per_image',
        'keep', 'K', 'out_img', 'out_xy', 'out_conf', 'out_cls', 'out_src', 'count_out', 'ws', 'err')


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name in ('cy_nms_boxes', 'cy_nms_max_per_image'):
        assert re.search(r'\bint %s\(' % name, header)
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert 'cy_nms_boxes' in _lib._SIGS and len(_lib._SIGS['cy_nms_boxes']) == len(ARGS) + 1
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6
    # 48 bytes of LDS per box: 160 KiB hold 3413 of them, far more than the 722 of a 19 x 19 grid with two boxes per cell
    assert _lib.query('cy_nms_max_per_image') == (160 * 1024) // 48 == 3413


def _args(**kw):
    """A call with plausible non-null pointers (never dereferenced on the host; the refusals come before the launch)."""
    a = dict(count_in=8, box_img=8, box_xy=8, conf=8, cls=8, n_cap=16, n_images=2, iou_th=0.45, class_aware=0, per_image=0,
             max_per_image=1024, keep=8, K=4, out_img=8, out_xy=8, out_conf=8, out_cls=8, out_src=8, count_out=8, ws=8, err=8)
    a.update(kw)
    return [a[k] for k in ARGS] + [None]


@pytest.mark.parametrize('kw,msg', [(dict(count_in=None), 'null argument'), (dict(keep=None), 'null argument'),
                                    (dict(count_out=None), 'null argument'), (dict(ws=None), 'null argument'),
                                    (dict(err=None), 'null argument'), (dict(box_img=None), 'null argument'),
                                    (dict(box_xy=None), 'null argument'), (dict(conf=None), 'null argument'),
                                    (dict(out_img=None), 'null argument'), (dict(out_xy=None), 'null argument'),
                                    (dict(out_conf=None), 'null argument'), (dict(out_src=None), 'null argument'),
                                    (dict(out_cls=None), 'null argument (out_cls'),
                                    (dict(K=-1), 'K=-1'), (dict(n_cap=-5), 'n_cap=-5'), (dict(n_images=0), 'n_images=0'),
                                    (dict(iou_th=float('nan')), 'iou_th=nan'), (dict(iou_th=1.5), 'iou_th=1.5'),
                                    (dict(iou_th=-0.1), 'iou_th=-0.1'), (dict(per_image=-2), 'per_image=-2'),
                                    (dict(class_aware=1, cls=None), 'class_aware=1 needs cls'),
                                    (dict(max_per_image=0), 'max_per_image=0'),
                                    (dict(max_per_image=3414), 'max_per_image=3414 needs 163872 bytes of LDS')])
def test_entry_point_refuses_bad_arguments(kw, msg):
    with pytest.raises(_lib.HipExtensionError, match='cy_nms_boxes: .*' + re.escape(msg)):
        _lib.call('cy_nms_boxes', *_args(**kw))


def test_entry_point_with_no_slots_or_no_entries_is_a_no_op():
    nothing = dict(box_img=None, box_xy=None, conf=None, cls=None, out_img=None, out_xy=None, out_conf=None, out_cls=None, out_src=None)
    _lib.call('cy_nms_boxes', *_args(K=0, **nothing))                    # nothing is launched
    _lib.call('cy_nms_boxes', *_args(n_cap=0, **nothing))
    _lib.call('cy_nms_boxes', *_args(K=0, max_per_image=3413, **nothing))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sorted(R.known_answers()))
def test_known_answers_of_the_restatement(name):
    kw, want = R.known_answers()[name]
    keep, order, visited, overflow = R.nms(**kw)
    assert keep.tolist() == want and overflow == 0
    conf, img = np.asarray(kw['conf'], np.float32), np.asarray(kw['box_img'])
    assert sorted(order.tolist()) == np.flatnonzero(keep).tolist()
    assert np.all(np.diff(img[order]) >= 0)                              # image ascending ...
    for b in set(img.tolist()):
        assert np.all(np.diff(conf[order][img[order] == b]) <= 0)        # ... and inside an image confidence descending


def test_the_threshold_case_sits_on_the_threshold():
    assert R.box_iou([0, 0, 3, 3], [0, 0, 4, 5]) == np.float64(9.0) / np.float64(20.0) == 0.45
    assert R.box_iou([0, 0, 5, 5], [5, 0, 10, 5]) == 0.0 and R.box_iou([0, 0, 5, 5], [6, 0, 10, 5]) == 0.0
    assert np.isnan(R.box_iou([3, 3, 3, 3], [3, 3, 3, 3]))               # two equal points: 0 / 0, and a NaN suppresses nothing
    assert R.nms([0, 0], [[3, 3, 3, 3], [3, 3, 3, 3]], [0.9, 0.8], iou_th=0.0)[0].tolist() == [1, 1]
    assert R.malformed(np.array([0.0, 0.0, np.inf, 1.0])) and R.malformed(np.array([2.0, 0.0, 1.0, 1.0]))
    assert not R.malformed(np.array([1.0, 1.0, 1.0, 1.0]))


def test_outputs_of_the_restatement():
    kw, _ = R.known_answers()['two_images']
    keep, order, _, _ = R.nms(**kw)
    count, o_img, o_xy, o_conf, o_cls, o_src = R.outputs(order, kw['box_img'], kw['box_xy'], kw['conf'], None, 3)
    assert count == 2 and o_src.tolist() == [0, 3, 0] and o_img.tolist() == [0, 2, 0] and o_cls is None
    assert o_xy.tolist() == [[0, 0, 10, 10], [1, 1, 9, 9], [0, 0, 0, 0]] and o_conf.tolist() == [np.float32(0.9), np.float32(0.95), 0.0]
    count, o_img, _, _, _, o_src = R.outputs(order, kw['box_img'], kw['box_xy'], kw['conf'], None, 1)
    assert count == 2 and o_src.tolist() == [0] and o_img.tolist() == [0]
    assert R.nms(max_per_image=1, **kw)[0].tolist() == [0, 0, 0, 0] and R.nms(max_per_image=1, **kw)[3] == 2


@pytest.mark.parametrize('seed', range(5))
@pytest.mark.parametrize('class_aware', [False, True])
def test_prefix_consistency_of_the_restatement(seed, class_aware):
    """Decoding at a higher threshold and suppressing gives the survivors of the full list that pass that threshold."""
    lists = [R.float_lists(seed), R.integer_lists([40, 0, 120], seed)]
    for img, xy, conf, cls in lists:
        full = R.nms(img, xy, conf, cls, n_images=3, iou_th=0.45, class_aware=class_aware)[0]
        assert 0 < full.sum() < len(full)
        for t in (0.0, 0.3, 0.5, 0.9):
            m = conf > np.float32(t)
            part = R.nms(img[m], xy[m], conf[m], cls[m], n_images=3, iou_th=0.45, class_aware=class_aware)[0]
            assert np.array_equal(full[m], part), t


@pytest.mark.parametrize('seed', range(5))
def test_the_float_lists_decide_nothing_on_the_threshold(seed):
    img, xy, conf, cls = R.float_lists(seed)
    keep, _, visited, _ = R.nms(img, xy, conf, cls, n_images=3, iou_th=0.45)
    assert len(img) == 400 and np.abs(visited - 0.45).min() >= 1e-9
    assert 0.15 * len(img) <= (keep == 0).sum() <= 0.4 * len(img)       # roughly a quarter is suppressed


# ------------------------------------------------------------------------------------------------ argument checks
def test_sign_detector_refuses_bad_nms_arguments():
    import types
    no_cls = types.SimpleNamespace(n_classes=0)
    for bad in (-0.1, 1.01, float('nan')):
        with pytest.raises(ValueError, match='nms_iou'):
            serve.SignDetector(None, None, None, None, nms_iou=bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='per_frame'):
            serve.SignDetector(None, None, None, None, nms_iou=0.45, per_frame=bad)
    with pytest.raises(ValueError, match='give nms_iou'):
        serve.SignDetector(None, None, None, None, per_frame=3)
    with pytest.raises(ValueError, match='give nms_iou'):
        serve.SignDetector(None, no_cls, None, None, nms_class_aware=True)
    with pytest.raises(ValueError, match='nms_class_aware needs a detector with class scores'):
        serve.SignDetector(None, no_cls, None, None, nms_iou=0.45, nms_class_aware=True)
    with pytest.raises(ValueError, match='max_boxes'):                   # the earlier check still comes first
        serve.SignDetector(None, None, None, None, max_boxes=0, nms_iou=7.0)


def test_wrappers_refuse_bad_arguments_before_any_device_work():
    import types
    from capsyolo_amd import predict_fns, utils
    with pytest.raises(ValueError, match='iou_th'):
        utils.nms_boxes_device([0], [[0, 0, 1, 1]], [0.5], iou_th=1.2)
    with pytest.raises(ValueError, match='per_image'):
        utils.nms_boxes_device([0], [[0, 0, 1, 1]], [0.5], per_image=-1)
    with pytest.raises(ValueError, match='needs the classes'):
        utils.nms_boxes_device([0], [[0, 0, 1, 1]], [0.5], class_aware=True)
    p0 = types.SimpleNamespace(n_classes=0)
    with pytest.raises(ValueError, match='n_classes > 0'):
        utils.nms_y_hat_device(np.zeros((1, 2, 2, 10), np.float32), p0, class_aware=True)
    with pytest.raises(ValueError, match='nms_iou'):
        predict_fns.dark_pred([], None, '', p0, 'last', nms_iou=2.0)
    with pytest.raises(ValueError, match='n_classes > 0'):
        predict_fns.dark_class_pred([], None, '', p0, None, '', None, 'last', nms_iou=0.5, nms_class_aware=True)
    with pytest.raises(ValueError, match='needs nms_iou'):
        predict_fns.dark_pred([], None, '', p0, 'last', nms_class_aware=True)


def _main():
    spec = importlib.util.spec_from_file_location('cy_main_nms_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_arguments_and_refusals():
    m = _main()
    a = m.parser.parse_args([])
    assert a.nms is None and a.nms_class_aware is False and a.per_frame == 0
    m.check_nms(a)
    serve_argv = ['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last']
    a = m.parser.parse_args(serve_argv + ['--nms', '0.45', '--nms_class_aware', '--per_frame', '3'])
    assert (a.nms, a.nms_class_aware, a.per_frame) == (0.45, True, 3)
    m.check_nms(a)
    m.check_nms(m.parser.parse_args(['--mode', 'detect', '--model', 'darknet_d', '--restore', 'last', '--nms', '0']))
    m.check_nms(m.parser.parse_args(['--mode', 'predict', '--model', 'darknet_r', '--combine', 'cnn', '--restore', 'last', '--nms', '1']))
    for argv, flag in ((['--mode', 'train', '--model', 'darknet_d', '--nms', '0.45'], '--nms'),
                       (['--mode', 'predict', '--model', 'capsule', '--restore', 'last', '--nms', '0.45'], '--nms'),
                       (['--mode', 'interpret', '--model', 'capsule', '--restore', 'last', '--nms', '0.45'], '--nms'),
                       (serve_argv + ['--nms', '1.5'], '--nms 1.5'), (serve_argv + ['--nms', '-0.2'], '--nms -0.2'),
                       (serve_argv + ['--nms', 'nan'], '--nms nan'),
                       (serve_argv + ['--nms_class_aware'], '--nms_class_aware'), (serve_argv + ['--per_frame', '2'], '--per_frame'),
                       (serve_argv + ['--nms', '0.45', '--per_frame', '-1'], '--per_frame -1'),
                       (['--mode', 'detect', '--model', 'darknet_d', '--restore', 'last', '--nms', '0.45', '--per_frame', '2'],
                        '--per_frame')):
        with pytest.raises(SystemExit, match=re.escape(flag)):
            m.main(argv)

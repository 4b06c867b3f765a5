"""CPU tests of the streaming detector (csrc/serve.hip, capsyolo_amd/serve.py, `main.py --mode serve`): the exports, the refusals
that come before any device work, the numpy restatement of tests/serve_ref.py against utils.crop_rectangles, and the CLI."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO

import serve_ref as R
from capsyolo_amd import _lib, serve, utils

NAMES = ('cy_boxes_crop_resize_u8', 'cy_pack_detections')


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\bint %s\(' % name, header)
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6


def _crop_args(**kw):
    """A call with plausible non-null pointers (never dereferenced on the host; the refusals come before the launch)."""
    a = dict(imgs=8, img_off=8, img_hw=8, n_images=1, imgs_bytes=48, count=8, box_img=8, box_xy=8, K=4, OH=8, OW=8, shift=0.0,
             scale=1.0, to_nchw=1, out=8, rect_out=8, err=8)
    a.update(kw)
    return [a[k] for k in ('imgs', 'img_off', 'img_hw', 'n_images', 'imgs_bytes', 'count', 'box_img', 'box_xy', 'K', 'OH', 'OW',
                           'shift', 'scale', 'to_nchw', 'out', 'rect_out', 'err')] + [None]


@pytest.mark.parametrize('kw,msg', [(dict(count=None), 'null argument'), (dict(out=None), 'null argument'),
                                    (dict(rect_out=None), 'null argument'), (dict(err=None), 'null argument'),
                                    (dict(K=-1), 'K=-1'), (dict(OH=0), 'output size 0 x 8'), (dict(OW=-3), 'output size 8 x -3'),
                                    (dict(box_xy=None), 'null argument'), (dict(imgs=None), 'null argument')])
def test_crop_entry_point_refuses_bad_arguments(kw, msg):
    with pytest.raises(_lib.HipExtensionError, match='cy_boxes_crop_resize_u8: .*' + re.escape(msg)):
        _lib.call('cy_boxes_crop_resize_u8', *_crop_args(**kw))


def test_crop_entry_point_with_no_slots_is_a_no_op():
    _lib.call('cy_boxes_crop_resize_u8', *_crop_args(K=0, imgs=None, box_img=None, box_xy=None))      # nothing is launched


@pytest.mark.parametrize('kw,msg', [(dict(count=None), 'null argument'), (dict(record=None), 'null argument'),
                                    (dict(K=-2), 'K=-2'), (dict(scores=None), 'null argument'), (dict(rect=None), 'null argument'),
                                    (dict(C=0), 'C=0'), (dict(record=12), '8-byte aligned')])
def test_pack_entry_point_refuses_bad_arguments(kw, msg):
    a = dict(scores=8, C=3, count=8, box_img=8, box_xy=8, conf=8, rect=8, crop_err=8, resize_err=8, K=4, record=8)
    a.update(kw)
    with pytest.raises(_lib.HipExtensionError, match='cy_pack_detections: .*' + re.escape(msg)):
        _lib.call('cy_pack_detections', *([a[k] for k in ('scores', 'C', 'count', 'box_img', 'box_xy', 'conf', 'rect', 'crop_err',
                                                          'resize_err', 'K', 'record')] + [None]))


def test_record_layout_mirrors_the_header():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    for cname, dtype in (('cy_detections_header_t', serve.HEADER_DTYPE), ('cy_detection_t', serve.RECORD_DTYPE)):
        body = re.search(r'typedef struct \{([^{}]*)\}\s*%s;' % cname, header, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [re.sub(r'\[\d+\]', '', d.split()[-1]) for d in body.split(';') if d.strip()]
        assert fields == list(dtype.names), cname
    assert serve.HEADER_DTYPE == R.HEADER_DTYPE and serve.RECORD_DTYPE == R.RECORD_DTYPE
    assert serve.HEADER_DTYPE.itemsize == 16 and serve.RECORD_DTYPE.itemsize == 48 and serve.record_bytes(16) == 16 + 48 * 16
    assert [serve.RECORD_DTYPE.fields[k][1] for k in serve.RECORD_DTYPE.names] == [0, 32, 36, 40, 44]
    with pytest.raises(ValueError):
        serve.unpack_record(np.zeros(10, np.uint8), 16)


RECT_HW = np.array([(37, 53), (20, 9)])
RECT_IDX = np.array([0, 0, 1, 1, 0, 1])
RECT_XY = np.array([[3.9, 4.2, 20.99, 30.0], [-7.5, -0.9, 12.3, 9.7], [2.0, 5.0, 30.0, 44.4], [-3.0, -3.0, 100.0, 100.0],
                    [52.2, 36.1, 60.0, 40.0], [0.5, 0.5, 1.5, 1.5]])


def test_restatement_agrees_with_the_rectangle_rule_on_accepted_boxes():
    want = utils.crop_rectangles(RECT_XY, RECT_IDX, RECT_HW)
    rect, bad, live = R.slot_rectangles(6, RECT_IDX, RECT_XY, RECT_HW, 8)
    assert np.array_equal(rect[:6], want) and not bad.any() and live.tolist() == [True] * 6 + [False] * 2
    assert not rect[6:].any()
    rect, bad, live = R.slot_rectangles(20, RECT_IDX, RECT_XY, RECT_HW, 4)                 # more boxes than slots
    assert np.array_equal(rect, want[:4]) and live.all() and not bad.any()
    rect, bad, live = R.slot_rectangles(0, RECT_IDX, RECT_XY, RECT_HW, 4)
    assert not rect.any() and not live.any() and not bad.any()


@pytest.mark.parametrize('box,idx', [([10.2, 5.0, 10.9, 9.0], 0), ([60.0, 5.0, 70.0, 9.0], 0), ([3.0, 8.0, 9.0, 8.5], 0),
                                     ([1.0, np.nan, 5.0, 5.0], 0), ([1.0, 1.0, np.inf, 5.0], 0), ([1.0, 1.0, 5.0, 5.0], 2),
                                     ([1.0, 1.0, 5.0, 5.0], -1)])
def test_restatement_marks_what_the_rectangle_rule_refuses(box, idx):
    xy = np.array([[1.0, 1.0, 5.0, 5.0], box])
    with pytest.raises(ValueError):
        utils.crop_rectangles(xy, np.array([0, idx]), RECT_HW)
    rect, bad, live = R.slot_rectangles(2, np.array([0, idx]), xy, RECT_HW, 3)
    assert rect.tolist() == [[1, 5, 1, 5], [0, 0, 0, 0], [0, 0, 0, 0]] and bad.tolist() == [False, True, False]


def test_pack_restatement():
    scores = np.array([[0.1, 0.7, 0.7], [np.nan, 2.0, 3.0], [5.0, 1.0, 0.0], [9.0, 9.0, 9.0]], dtype=np.float32)
    rect = np.array([[1, 5, 1, 5], [0, 2, 0, 2], [0, 0, 0, 0], [1, 2, 1, 2]])
    buf = R.pack(scores, 7, [0, 1, 0, 1], np.arange(16.0).reshape(4, 4), [0.9, 0.8, 0.7, 0.6], rect, 1, 0, 4)
    head, rec = serve.unpack_record(buf, 4)
    assert (int(head['total']), int(head['kept']), int(head['crop_err']), int(head['resize_err'])) == (7, 4, 1, 0)
    assert rec['cls'].tolist() == [1, 0, -1, 0] and rec['image'].tolist() == [0, 1, 0, 1]
    assert rec['score'][0] == np.float32(0.7) and np.isnan(rec['score'][1]) and rec['score'][2] == 0
    res = serve.Detections(buf, 4)
    assert res.n == 4 and res.total == 7 and res.truncated and res.bad == {'boxes': 1, 'frames': 0}
    assert res.boxes_xy.dtype == np.float64 and res.boxes_xy.shape == (4, 4) and res.classes.dtype == np.int64
    assert res.conf.dtype == np.float32 and res.class_scores.dtype == np.float32 and res.image_indices.dtype == np.int64
    two = serve.Detections(R.pack(scores, 2, [0, 1, 0, 1], np.zeros((4, 4)), np.zeros(4), rect, 0, 0, 4), 4)
    assert two.n == 2 and not two.truncated and two.classes.tolist() == [1, 0]


def test_sign_detector_refuses_to_run_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)          # (the same question on a machine that has one)
    with pytest.raises(_lib.HipExtensionError, match='no CPU path'):
        serve.SignDetector(None, None, None, None)


def test_sign_detector_refuses_a_bad_slot_count_and_bad_frames():
    for k in (0, -3, 2.5):
        with pytest.raises(ValueError, match='max_boxes'):
            serve.SignDetector(None, None, None, None, max_boxes=k)
    ok = np.zeros((4, 6, 3), np.uint8)
    assert len(serve.SignDetector._frames(ok)) == 1 and len(serve.SignDetector._frames(np.stack([ok, ok]))) == 2
    for frames in (np.zeros((4, 6, 3), np.float32), np.zeros((4, 6), np.uint8), [np.zeros((4, 6, 4), np.uint8)], []):
        with pytest.raises(ValueError):
            serve.SignDetector._frames(frames)
    with pytest.raises(ValueError, match='one size'):
        serve.SignDetector._frames([ok, np.zeros((4, 7, 3), np.uint8)])


def _main():
    spec = importlib.util.spec_from_file_location('cy_main_serve_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_arguments_and_refusals():
    m = _main()
    assert m.parser.parse_args([]).max_boxes == 16
    a = m.parser.parse_args(['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last', '--max_boxes', '4',
                             '--graph', '--synthetic', '3'])
    assert (a.mode, a.max_boxes, a.graph, a.combine, a.synthetic) == ('serve', 4, True, 'capsule', 3)
    m.check_serve(a)
    for argv in (['--mode', 'serve', '--model', 'darknet_d', '--restore', 'last'],
                 ['--mode', 'serve', '--model', 'capsule', '--combine', 'capsule', '--restore', 'last'],
                 ['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule'],
                 ['--mode', 'serve', '--model', 'darknet_r', '--combine', 'cnn', '--restore', 'best', '--max_boxes', '0']):
        with pytest.raises(SystemExit):
            m.main(argv)

"""CPU tests of the two-stage prediction chain: the numpy restatements of tests/pipeline_ref.py (the yardsticks of
tests/test_gpu_pipeline.py) against what the reference's own functions returned (tests/golden/pipeline.npz), and the host-side
rectangle rule of the product."""
import numpy as np
import pytest

from helpers import load_golden

import pipeline_ref as R
from capsyolo_amd import _lib, utils


@pytest.fixture(scope='module')
def gold():
    return load_golden('pipeline')


@pytest.mark.parametrize('tag', ['map_a', 'map_b'])
def test_sweep_restatement_reproduces_the_reference_mAP_exactly(gold, tag):
    y, y_hat = gold[tag + '_y'], gold[tag + '_y_hat']
    mAP, table = R.detect_and_recog_mAP(y, y_hat, int(gold[tag + '_side']))
    assert np.array_equal(table, gold[tag + '_ap_table'])
    assert mAP == float(gold[tag + '_mAP'])
    assert 0.1 < mAP < 0.9 and len(np.unique(table)) >= 5                       # the fixture is not a degenerate case


@pytest.mark.parametrize('tag', ['map_a', 'map_b'])
def test_sweep_restatement_at_one_threshold_is_the_existing_confusion(gold, tag):
    from oracle import utils_np
    y, y_hat, side = gold[tag + '_y'], gold[tag + '_y_hat'], int(gold[tag + '_side'])
    counts = R.confusion_sweep(y, y_hat, 43, side, [0.5], [0.5])
    assert counts.shape == (1, 43, 1, 3)
    assert list(counts.sum(axis=(0, 1, 2))) == [int(v) for v in utils_np.detect_and_recog_confusion(y, y_hat, 43, side)]
    assert utils_np.detect_and_recog_acc(y, y_hat, 43, side) == float(gold[tag + '_f1'])


def test_combine_restatement_equals_the_reference(gold):
    out = R.combine_y_hat(gold['combine_image_hw'], gold['combine_dark'], gold['combine_scores'], gold['combine_idx'],
                          gold['combine_xy'], int(gold['combine_side']), 3)
    assert out.dtype == np.float64 and np.array_equal(out, gold['combine_y_hat'])
    row, col = R.box_cells(gold['combine_image_hw'], gold['combine_idx'], gold['combine_xy'], int(gold['combine_side']), 3)
    cells = list(zip(gold['combine_idx'].tolist(), row.tolist(), col.tolist()))
    assert len(cells) - len(set(cells)) >= 3                                     # boxes that land in an already written cell


def test_combine_restatement_refuses_a_box_outside_the_grid(gold):
    xy = gold['combine_xy'].copy()
    xy[0, [0, 2]] += 1000.0
    with pytest.raises(ValueError):
        R.combine_y_hat(gold['combine_image_hw'], gold['combine_dark'], gold['combine_scores'], gold['combine_idx'], xy,
                        int(gold['combine_side']), 3)


RECT_HW = np.array([(37, 53), (20, 9)])
RECT_IDX = np.array([0, 0, 1, 1, 0, 1])
RECT_XY = np.array([[3.9, 4.2, 20.99, 30.0],        # plain truncation
                    [-7.5, -0.9, 12.3, 9.7],        # negative corners: -0.9 truncates to 0, -7.5 is clipped (no wrap-around)
                    [2.0, 5.0, 30.0, 44.4],         # beyond the right and bottom border
                    [-3.0, -3.0, 100.0, 100.0],     # the whole image
                    [52.2, 36.1, 60.0, 40.0],       # the last column and row only
                    [0.5, 0.5, 1.5, 1.5]])          # one pixel


def test_rectangle_rule_equals_the_restatement():
    rect = utils.crop_rectangles(RECT_XY, RECT_IDX, RECT_HW)
    assert rect.dtype == np.int64 and np.array_equal(rect, R.crop_rectangles(RECT_XY, RECT_IDX, RECT_HW))
    assert rect.tolist() == [[4, 30, 3, 20], [0, 9, 0, 12], [5, 20, 2, 9], [0, 20, 0, 9], [36, 37, 52, 53], [0, 1, 0, 1]]


@pytest.mark.parametrize('box', [[10.2, 5.0, 10.9, 9.0], [60.0, 5.0, 70.0, 9.0], [-9.0, 5.0, -2.0, 9.0], [3.0, 8.0, 9.0, 8.5]])
def test_empty_rectangle_raises_and_names_the_box(box):
    xy = np.array([[1.0, 1.0, 5.0, 5.0], box])
    with pytest.raises(ValueError, match='box 1 of image 0'):
        utils.crop_rectangles(xy, np.array([0, 0]), RECT_HW)
    with pytest.raises(ValueError):
        R.crop_rectangles(xy, np.array([0, 0]), RECT_HW)


def test_bilinear_restatement_known_answers():
    img = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    same = R.crop_resize(img, (0, 4, 0, 6), 4, 6)
    assert np.array_equal(same, img.astype(np.float64))                          # same size: the identity
    half = R.crop_resize(img, (0, 4, 0, 6), 2, 3)                                # exact 2x2 box means
    assert np.allclose(half, img.astype(np.float64).reshape(2, 2, 3, 2, 3).mean(axis=(1, 3)), atol=1e-12)
    up = R.crop_resize(img, (1, 2, 2, 3), 5, 5, -128.0, 1.0 / 128.0)             # one pixel: constant, then centred
    assert np.allclose(up, (img[1, 2].astype(np.float64) - 128.0) / 128.0)


def test_new_entry_points_are_exported():
    lib = _lib.load()
    for name in ('cy_crop_resize_u8', 'cy_combine_scores', 'cy_yolo_decode_boxes_conf', 'cy_confusion_sweep'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 6

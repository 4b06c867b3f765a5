"""GPU tests of the two-stage prediction chain (csrc/predict.hip behind predict_fns / utils / metrics): crop + resize, the
combine step, the one-launch threshold sweep and detect_and_recog_mAP, dark_class_pred and `main.py --mode predict` end to end.
The yardsticks are the numpy restatements of tests/pipeline_ref.py (pinned against the reference by tests/test_pipeline_host.py)
and tests/golden/pipeline.npz, which holds what the reference's own functions returned."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, load_golden, make_params

import pipeline_ref as R
from capsyolo_amd import metrics, models, predict_fns, synth, utils
from oracle import utils_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return load_golden('pipeline')


# ------------------------------------------------------------------------------------------------ crop + resize
def _two_images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (20, 9, 3), dtype=np.uint8)]


CROP_IMG = np.array([0, 1, 0, 0, 1, 0, 1])
CROP_RECT = np.array([[0, 37, 0, 53],        # whole image (a downscale at 16 x 16)
                      [0, 20, 0, 9],         # whole second image: up in x, down or up in y
                      [11, 16, 20, 27],      # 5 x 7 crop: edge clamping on every side when it goes up to 32 x 32
                      [3, 30, 17, 18],       # one pixel wide
                      [4, 20, 8, 9],         # one pixel wide at the right border, down to the bottom border
                      [25, 37, 40, 53],      # touches the right and the bottom border
                      [19, 20, 0, 9]])       # one pixel high, the last row


def crop_bound(scale):
    """fp32 weight (one rounding: the coordinate is an exact fraction), two lerps of three roundings each and the affine, on
    values <= 255: at most 8 half-ulps-of-256, 8 * 2^-24 * 255, times the scale."""
    return 8 * 2.0 ** -24 * 255 * scale


@pytest.mark.parametrize('side', [16, 32])
@pytest.mark.parametrize('to_nchw', [False, True])
@pytest.mark.parametrize('shift,scale', [(0.0, 1.0), (-128.0, 1.0 / 128.0)])
def test_crop_resize_against_fp64(side, to_nchw, shift, scale):
    images = _two_images()
    packed = predict_fns.PackedImages(images)
    out = packed.crop_resize(CROP_IMG, CROP_RECT, side, side, shift, scale, to_nchw).cpu().numpy()
    assert out.shape == ((len(CROP_IMG), 3, side, side) if to_nchw else (len(CROP_IMG), side, side, 3))
    if to_nchw:
        out = out.transpose(0, 2, 3, 1)
    worst = 0.0
    for b in range(len(CROP_IMG)):
        ref = R.crop_resize(images[CROP_IMG[b]], CROP_RECT[b], side, side, shift, scale)
        worst = max(worst, float(np.abs(out[b].astype(np.float64) - ref).max()))
    print('crop_resize side %d nchw %d scale %g: max abs error %.3g (bound %.3g)' % (side, to_nchw, scale, worst, crop_bound(scale)))
    assert worst <= crop_bound(scale)


def test_crop_resize_rectangular_output_and_identity():
    images = _two_images()
    packed = predict_fns.PackedImages(images)
    same = packed.crop_resize([1], [[0, 20, 0, 9]], 20, 9).cpu().numpy()[0]
    assert np.array_equal(same, images[1].astype(np.float32))                    # same size: every weight is 0
    out = packed.crop_resize([0, 0], [[0, 37, 0, 53], [2, 9, 1, 50]], 7, 19).cpu().numpy()
    for b, rect in enumerate([[0, 37, 0, 53], [2, 9, 1, 50]]):
        assert np.abs(out[b] - R.crop_resize(images[0], rect, 7, 19)).max() <= crop_bound(1.0)


def test_crop_resize_refuses_a_rectangle_outside_its_image():
    packed = predict_fns.PackedImages(_two_images())
    for img, rect in ((1, [0, 21, 0, 9]), (1, [0, 20, 0, 10]), (0, [5, 5, 0, 9]), (0, [-1, 5, 0, 9]), (2, [0, 5, 0, 5])):
        with pytest.raises(ValueError):
            packed.crop_resize([img], [rect], 8, 8)


def test_rectangle_rule_and_empty_rectangle():
    hw = np.array([(37, 53), (20, 9)])
    xy = np.array([[-7.5, -0.9, 12.3, 9.7], [2.0, 5.0, 30.0, 44.4], [52.2, 36.1, 60.0, 40.0]])
    idx = np.array([0, 1, 0])
    rect = utils.crop_rectangles(xy, idx, hw)
    assert np.array_equal(rect, R.crop_rectangles(xy, idx, hw)) and rect.tolist() == [[0, 9, 0, 12], [5, 20, 2, 9], [36, 37, 52, 53]]
    with pytest.raises(ValueError, match='box 1 of image 0'):
        utils.crop_rectangles(np.array([[1.0, 1.0, 5.0, 5.0], [60.0, 5.0, 70.0, 9.0]]), np.array([0, 0]), hw)


# ------------------------------------------------------------------------------------------------ combine
def test_combine_y_hat_equals_the_reference_and_is_deterministic(gold):
    p = make_params(n_classes=0, n_grid=3, darknet_input=int(gold['combine_side']))
    args = (gold['combine_image_hw'], gold['combine_dark'], gold['combine_scores'], gold['combine_idx'], gold['combine_xy'], p)
    out = utils.combine_y_hat(*args)
    assert out.dtype == np.float64 and out.shape == gold['combine_y_hat'].shape
    assert np.array_equal(out, gold['combine_y_hat'])
    assert np.array_equal(utils.combine_y_hat(*args), out)                       # duplicates are decided by index, not by timing
    images = [np.zeros((h, w, 3), dtype=np.uint8) for h, w in gold['combine_image_hw']]
    assert np.array_equal(utils.combine_y_hat(images, *args[1:]), out)           # the reference's first argument: the images


def test_combine_y_hat_without_boxes_and_outside_the_grid(gold):
    p = make_params(n_classes=0, n_grid=3, darknet_input=int(gold['combine_side']))
    dark, hw = gold['combine_dark'], gold['combine_image_hw']
    out = utils.combine_y_hat(hw, dark, np.zeros((0, 43), np.float32), np.zeros(0, np.int64), np.zeros((0, 4)), p)
    assert np.array_equal(out[..., :10], dark.astype(np.float64)) and not out[..., 10:].any()
    xy = gold['combine_xy'].copy()
    xy[3, [0, 2]] += 1000.0
    with pytest.raises(ValueError):
        utils.combine_y_hat(hw, dark, gold['combine_scores'], gold['combine_idx'], xy, p)


# ------------------------------------------------------------------------------------------------ sweep and mAP
@pytest.mark.parametrize('tag', ['map_a', 'map_b'])
def test_confusion_sweep_and_mAP_against_the_reference(gold, tag):
    y, y_hat, side = gold[tag + '_y'], gold[tag + '_y_hat'], int(gold[tag + '_side'])
    p = make_params(n_classes=43, darknet_input=side)
    counts = metrics.confusion_sweep(y, y_hat, p, R.MAP_CONF_THS, R.MAP_IOU_THS)
    assert counts.dtype == np.int64 and counts.shape == (100, 43, 10, 3)
    assert np.array_equal(counts, R.confusion_sweep(y, y_hat, 43, side, R.MAP_CONF_THS, R.MAP_IOU_THS))
    assert np.array_equal(metrics._ap_table(counts), gold[tag + '_ap_table'])
    p0 = make_params(n_classes=0, darknet_input=side)                            # the metric forces 43 classes like the reference
    mAP = metrics.detect_and_recog_mAP(y, y_hat, p0)
    print('%s: mAP %.17g (reference %.17g)' % (tag, mAP, float(gold[tag + '_mAP'])))
    assert p0.n_classes == 43 and abs(mAP - float(gold[tag + '_mAP'])) <= 1e-12
    assert abs(metrics.detect_and_recog_mAP(torch.from_numpy(y).cuda(), torch.from_numpy(y_hat).cuda(), p0) - mAP) == 0.0


@pytest.mark.parametrize('tag', ['map_a', 'map_b'])
def test_confusion_sweep_agrees_with_the_existing_metrics(gold, tag):
    y, y_hat, side = gold[tag + '_y'], gold[tag + '_y_hat'], int(gold[tag + '_side'])
    p = make_params(n_classes=43, darknet_input=side)
    one = metrics.confusion_sweep(y, y_hat, p, [0.5], [0.5])
    assert one.shape == (1, 43, 1, 3)
    assert list(one.sum(axis=(0, 1, 2))) == list(metrics.detect_and_recog_confusion(y, y_hat, p))
    # class-agnostic table -> detect_AP (which strips nothing: give it arrays without class scores)
    nb = (y_hat.shape[3] - 43) // 5
    y5, h5 = np.ascontiguousarray(y[..., :5]), np.ascontiguousarray(y_hat[..., :5 * nb])
    p0 = make_params(n_classes=0, darknet_input=side)
    flat = metrics.confusion_sweep(y5, h5, p0, R.MAP_CONF_THS, R.MAP_IOU_THS, per_class=False)
    assert flat.shape == (100, 1, 10, 3)
    assert np.array_equal(flat, R.confusion_sweep(y5, h5, 0, side, R.MAP_CONF_THS, R.MAP_IOU_THS, per_class=False))
    assert np.mean(metrics._ap_table(flat)[0]) == metrics.detect_AP(y5, h5, p0)


@pytest.mark.parametrize('seed,B,g,nb,C,per_class', [(21, 3, 5, 2, 43, True),      # two boxes per cell
                                                     (22, 2, 5, 2, 2, True),       # two classes: a group holds more boxes than a wavefront
                                                     (23, 2, 5, 2, 2, False),      # one group per image: 50 predictions + ground truth
                                                     (24, 2, 12, 2, 3, False)])    # 288 predictions in a group: more than the block's 256 threads
def test_confusion_sweep_seeded_cases(seed, B, g, nb, C, per_class):
    y, y_hat = R.sweep_case(seed, B, g, nb, C, mark_frac=0.6 if g == 5 else 0.45)
    p = make_params(n_classes=C, darknet_input=416)
    conf_ths, iou_ths = np.linspace(0, 1, 23), np.array([0.3, 0.5, 0.75, 0.9])
    ref = R.confusion_sweep(y, y_hat, C, 416, conf_ths, iou_ths, per_class)
    out = metrics.confusion_sweep(y, y_hat, p, conf_ths, iou_ths, per_class)
    assert ref[..., 0].max() > 0 and np.array_equal(out, ref)
    # thresholds in another order land in the matching rows (nothing assumes that they ascend)
    perm = np.random.default_rng(seed).permutation(len(conf_ths))
    assert np.array_equal(metrics.confusion_sweep(y, y_hat, p, conf_ths[perm], iou_ths[::-1], per_class), ref[perm][:, :, ::-1])


def test_confusion_sweep_empty_sides():
    y, y_hat = R.sweep_case(31, 2, 4, 1, 43)
    p = make_params(n_classes=43, darknet_input=416)
    ths = (np.linspace(0, 1, 5), np.array([0.5, 0.75]))
    present = y[..., 5:].reshape(-1, 43).sum(0) > 0
    assert 0 < present.sum() < 43                                                # classes without a ground-truth box
    out = metrics.confusion_sweep(y, y_hat, p, *ths)
    assert np.array_equal(out, R.confusion_sweep(y, y_hat, 43, 416, *ths))
    assert not out[:, ~present, :, 0].any() and not out[:, ~present, :, 2].any() and out[0, :, :, 0].sum() > 0
    quiet = y_hat.copy()
    quiet[..., 0] = 0.0                                                          # no prediction over the lowest threshold
    out = metrics.confusion_sweep(y, quiet, p, *ths)
    assert np.array_equal(out, R.confusion_sweep(y, quiet, 43, 416, *ths))
    assert not out[..., 0].any() and not out[..., 1].any() and out[0, :, 0, 2].sum() == int(y[..., 0].sum())
    none = np.zeros_like(y)                                                      # no ground truth at all
    out = metrics.confusion_sweep(none, y_hat, p, *ths)
    assert np.array_equal(out, R.confusion_sweep(none, y_hat, 43, 416, *ths)) and not out[..., 0].any() and out[..., 1].any()


def test_confusion_sweep_reports_a_malformed_box():
    y, y_hat = R.sweep_case(32, 1, 3, 1, 2, mark_frac=1.0)
    y_hat[0, 0, 0, 3] = -0.2                                                     # negative width: x1 > x2
    with pytest.raises(AssertionError):
        metrics.confusion_sweep(y, y_hat, make_params(n_classes=2, darknet_input=416), [0.0, 0.5], [0.5])


def test_confusion_sweep_refuses_a_grid_that_does_not_fit_the_lds():
    from capsyolo_amd._lib import HipExtensionError
    y, y_hat = np.zeros((1, 40, 40, 7)), np.zeros((1, 40, 40, 12), dtype=np.float32)      # 3200 boxes per group: 486 KB
    with pytest.raises(HipExtensionError, match='LDS'):
        metrics.confusion_sweep(y, y_hat, make_params(n_classes=2, darknet_input=416), R.MAP_CONF_THS, R.MAP_IOU_THS)


# ------------------------------------------------------------------------------------------------ end to end
IMAGE_HW = [(80, 120), (64, 64), (100, 70)]


def _images():
    out = []
    for k, (h, w) in enumerate(IMAGE_HW):
        rng = np.random.default_rng(100 + k)
        ramp = np.add.outer(np.linspace(0, 120, h), np.linspace(0, 100, w))[:, :, None]
        out.append(np.clip(ramp + rng.integers(0, 36, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def _checkpoints(tmp_path):
    dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    cp = make_params(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(3)
    dark = models.DarkNet(dp)
    caps = models.CapsuleNet(cp)
    ddir, cdir = str(tmp_path / 'darknet_d'), str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': dark.state_dict()}, False, ddir)
    utils.save_checkpoint({'epoch': 0, 'state_dict': caps.state_dict()}, False, cdir)
    return dp, cp, ddir, cdir


def test_resize_images_device_against_fp64():
    images = _images()
    out = predict_fns.resize_images_device(images, 64)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (3, 3, 64, 64)
    out = out.cpu().numpy().transpose(0, 2, 3, 1)
    for k, im in enumerate(images):
        err = np.abs(out[k] - R.crop_resize(im, (0, im.shape[0], 0, im.shape[1]), 64, 64)).max()
        assert err <= crop_bound(1.0), (k, err)
    assert np.array_equal(out[1], images[1].astype(np.float32))                  # 64 x 64 stays as it is


def test_dark_class_pred_end_to_end(tmp_path):
    images = _images()
    dp, cp, ddir, cdir = _checkpoints(tmp_path)
    dark, caps = models.DarkNet(dp).cuda(), models.CapsuleNet(cp).cuda()
    # a confidence threshold that lets some, not all, boxes through: halfway between two neighbouring confidences of the same
    # forward (chunks of 2 images, like the call below: an untrained detector's confidences lie close together)
    y0, drawn = predict_fns.dark_pred(images, dark, ddir, dp, 'last', batch_size=2)
    assert drawn is None and y0.shape == (3, 2, 2, 10)
    conf = np.unique(y0[..., 0::5])[::-1].astype(np.float64)
    print('confidences: %s' % conf)
    assert len(conf) >= 8, 'the detector output has too few distinct confidences: %s' % conf
    conf_th = float(conf[5] + conf[6]) / 2                                       # distinct values: several boxes may share one
    y_hat, none = predict_fns.dark_class_pred(images, dark, ddir, dp, caps, cdir, cp, 'last', batch_size=2, conf_th=conf_th)
    assert none is None and y_hat.dtype == np.float64 and y_hat.shape == (3, 2, 2, 53)
    dark_part = y_hat[..., :10].astype(np.float32)
    assert np.array_equal(dark_part, y0)
    y32, _ = predict_fns.dark_pred(images, dark, ddir, dp, 'last')               # all images in one chunk: the same forward
    np.testing.assert_allclose(y32, y0, rtol=1e-4, atol=1e-5)
    # everything behind the detector once more with the restatements (and class_pred for the classifier's forward)
    hw = np.array(IMAGE_HW)
    idx, xy, _ = utils_np.y_to_boxes_vec(dark_part, 0, 64, hw, conf_th)
    occupied = (y_hat[..., 10:] != 0).any(axis=-1)
    print('conf_th %.6f: %d boxes, %d of 12 cells with class scores' % (conf_th, len(idx), occupied.sum()))
    assert 4 <= len(idx) < 24 and not occupied.all() and occupied.any()      # some boxes, not all; a cell without a box
    rect = R.crop_rectangles(xy, idx, hw)
    crops = np.stack([R.crop_resize(images[i], r, 32, 32, -128.0, 1.0 / 128.0) for i, r in zip(idx, rect)]).astype(np.float32)
    scores, _ = predict_fns.class_pred(crops, caps, cdir, cp, 'last')
    ref = R.combine_y_hat(hw, dark_part, scores, idx, xy, 64, 2)
    err = np.abs(y_hat - ref).max()
    print('combined y_hat: max abs difference %.3g' % err)
    assert err <= 2e-4
    # dark_pred's detached outputs: raw-scale crops, indices and boxes of the same decode
    y1, raw, idx1, xy1 = predict_fns.dark_pred(images, dark, ddir, dp, 'last', is_end=False, conf_th=conf_th, batch_size=2)
    assert np.array_equal(y1, dark_part) and np.array_equal(idx1, idx)
    np.testing.assert_allclose(xy1, xy, rtol=1e-14, atol=1e-11)
    assert raw.dtype == np.float32 and raw.shape == (len(idx), 32, 32, 3)
    assert np.abs(raw - (crops.astype(np.float64) * 128.0 + 128.0)).max() <= 1e-3
    # no box at all is a valid outcome: the class part stays zero
    y_none, _ = predict_fns.dark_class_pred(images, dark, ddir, dp, caps, cdir, cp, 'last', batch_size=2, conf_th=2.0)
    assert np.array_equal(y_none[..., :10].astype(np.float32), y0) and not y_none[..., 10:].any()


def test_main_predict_mode_writes_both_metrics(tmp_path):
    _, _, ddir, cdir = _checkpoints(tmp_path)
    json.dump(dict(batch_size=4, n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, dropout=0.0),
              open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_predict', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(['--mode', 'predict', '--model', 'darknet_d', '--combine', 'capsule', '--synthetic', '6', '--model_dir', ddir,
                  '--restore', 'last'])
    text = open(os.path.join(ddir, 'combine-capsule_metric_output.txt')).read()
    fields = dict(f.split(':') for f in text.split(', ') if f)
    assert list(fields) == ['detect_and_recog_mAP', 'detect_and_recog_acc'] == list(out)
    for k, v in fields.items():
        assert np.isfinite(float(v)) and float(v) == float(out[k]) and 0.0 <= float(v) <= 1.0
    with pytest.raises(SystemExit):
        m.main(['--mode', 'predict', '--model', 'darknet_d', '--synthetic', '6', '--model_dir', ddir, '--restore', 'last'])

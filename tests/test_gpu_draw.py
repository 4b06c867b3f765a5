"""GPU tests of box drawing: the rasteriser `cy_draw_boxes_u8` (csrc/draw.hip) behind capsyolo_amd.draw, the `draw=True` paths of
predict_fns.dark_pred / dark_class_pred, metrics.detect_report and `main.py --mode detect` / `--draw` end to end.  The yardstick is
the sequential numpy restatement tests/draw_ref.py (pinned against hand-written pixel sets by tests/test_draw_host.py); every
comparison is exact byte equality."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, make_params

import pipeline_ref as R
from capsyolo_amd import _lib, draw, metrics, models, predict_fns, synth, utils
from capsyolo_amd.interpret import read_ppm
from draw_ref import draw_ref
from oracle import utils_np

pytestmark = pytest.mark.gpu

GLYPHS = draw.DIGITS_5X7
BLUE = (255, 0, 0)
# (height, width): the three sizes, and a second 7 x 9 image (index 2) that never gets a box
SIZES = [(1, 1), (7, 9), (7, 9), (64, 48)]
BIG = 3


def _canvas():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


# (image, x1, y1, x2, y2, label, colour); the images interleaved, so the wrapper's stable sort by image has work to do
BOXES = [
    (BIG, 5, 6, 20, 30, -1, draw.GREEN),              # interior
    (0, 0, 0, 0, 0, -1, draw.RED),                    # the 1 x 1 image: its only pixel
    (BIG, -4, 10, 8, 20, 0, BLUE),                    # crosses the left border; label 0
    (1, 1, 1, 7, 5, 42, draw.GREEN),                  # the 7 x 9 image: label 42 at (4, 3), cut by the top and the right border
    (BIG, 10, -5, 25, 9, 42, draw.RED),               # crosses the top border
    (BIG, 40, 12, 55, 28, 999, draw.GREEN),           # crosses the right border; the label 999 too
    (0, -3, -3, 5, 5, 8, BLUE),                       # around the 1 x 1 image: draws nothing
    (BIG, 12, 50, 30, 70, -1, BLUE),                  # crosses the bottom border
    (BIG, 100, 100, 120, 130, 5, draw.RED),           # wholly outside, label and all
    (BIG, -10, -10, 60, 80, 7, draw.RED),             # larger than the image: only its label at (25, 35) shows
    (1, 8, 6, 8, 6, -1, BLUE),                        # a single point in the bottom-right corner of the 7 x 9 image
    (BIG, 33, 44, 33, 44, -1, draw.GREEN),            # a single point
    (BIG, 30, 40, 22, 33, 3, BLUE),                   # inverted
    (BIG, 44, 60, 49, 71, 88, draw.GREEN),            # label at (46, 65): cut by the bottom-right corner
    (BIG, -13, 20, 10, 31, 1, draw.RED),              # text origin x = (-13 + 10) // 2 = -2: floor, not truncation
]


def _split(boxes):
    idx = np.array([b[0] for b in boxes], dtype=np.int64)
    xy = np.array([b[1:5] for b in boxes], dtype=np.int64).reshape(-1, 4)
    lab = np.array([b[5] for b in boxes], dtype=np.int64)
    col = np.array([b[6] for b in boxes], dtype=np.uint8).reshape(-1, 3)
    return idx, xy, lab, col


def _draw(packed, boxes, with_labels=True):
    idx, xy, lab, col = _split(boxes)
    buf = draw.draw_boxes_device(packed, idx, xy.astype(np.float64), col, lab if with_labels else None)
    assert buf.dtype == torch.uint8 and buf.is_cuda and buf.shape == packed.buf.shape and buf.data_ptr() != packed.buf.data_ptr()
    return draw.unpack_images(buf, packed)


def _ref(images, boxes, with_labels=True):
    idx, xy, lab, col = _split(boxes)
    return draw_ref(images, idx, xy, col, lab if with_labels else None, GLYPHS)


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the kernel
def test_kernel_equals_the_sequential_restatement():
    images = _canvas()
    packed = predict_fns.PackedImages(images)
    out, ref = _draw(packed, BOXES), _ref(images, BOXES)
    assert _same(out, ref)
    assert np.array_equal(out[2], images[2]) and not np.array_equal(out[BIG], images[BIG])      # the image without a box
    assert tuple(out[0][0, 0]) == draw.RED                                                      # the 1 x 1 image
    assert tuple(out[1][6, 8]) == BLUE and tuple(out[BIG][44, 33]) == draw.GREEN                 # the single points
    assert _same(_draw(packed, BOXES, with_labels=False), _ref(images, BOXES, with_labels=False))
    assert not _same(out, _ref(images, BOXES, with_labels=False))                               # the labels are there


CROSSING = [(BIG, 4, 4, 30, 30, 12, draw.GREEN),      # edges cross the next box's edges, the label '12' at (17, 17) its left edge
            (BIG, 18, 10, 40, 24, 345, draw.RED),     # label '345' at (29, 17) crosses the first box's right edge x = 30
            (BIG, 10, 12, 36, 20, 6, BLUE)]           # label '6' at (23, 16) overlaps the '12'; its edges cross both boxes


@pytest.mark.parametrize('count', [2, 3])
def test_the_later_box_wins(count):
    images = _canvas()
    packed = predict_fns.PackedImages(images)
    boxes = CROSSING[:count]
    fwd, rev = _draw(packed, boxes), _draw(packed, boxes[::-1])
    assert _same(fwd, _ref(images, boxes)) and _same(rev, _ref(images, boxes[::-1]))
    assert not np.array_equal(fwd[BIG], rev[BIG])
    assert tuple(fwd[BIG][10, 30]) == draw.RED and tuple(rev[BIG][10, 30]) == draw.GREEN         # where x = 30 meets y = 10


def _crowd():
    rng = np.random.default_rng(2024)
    extra = []
    for _ in range(60):
        x1, x2 = (int(v) for v in rng.integers(-6, 54, 2))
        y1, y2 = (int(v) for v in rng.integers(-6, 70, 2))
        extra.append((BIG, x1, y1, x2, y2, int(rng.integers(-1, 1000)), (draw.GREEN, draw.RED, BLUE)[int(rng.integers(0, 3))]))
    return BOXES + extra


def test_four_runs_give_the_same_bytes_and_nothing_else_is_touched():
    images = _canvas()
    packed = predict_fns.PackedImages(images)
    before = packed.buf.clone()
    boxes = _crowd()
    runs = [_draw(packed, boxes) for _ in range(4)]
    assert all(_same(runs[0], r) for r in runs[1:])
    assert torch.equal(packed.buf, before)                                                      # the source buffer
    assert _same(runs[0], _ref(images, boxes))
    idx, xy, lab, _ = _split(boxes)
    white = np.full((len(boxes), 3), 255, dtype=np.uint8)
    touched = draw_ref([np.zeros_like(im) for im in images], idx, xy, white, lab, GLYPHS)
    for out, im, t in zip(runs[0], images, touched):
        keep = ~t.any(axis=2)
        assert np.array_equal(out[keep], im[keep])
    assert touched[BIG].any(axis=2).sum() > 1500                                                # a crowd indeed


def _raw_launch(packed, boxes):
    """The C-ABI call itself, boxes as given (so: image index ascending): (images, error count)."""
    idx, xy, lab, col = _split(boxes)
    n = len(boxes)
    out = packed.buf.clone()
    words = torch.from_numpy(np.concatenate([idx, xy.reshape(-1), lab, [0]]).astype(np.int32)).cuda()
    cols = torch.from_numpy(col.copy()).cuda()
    glyphs = torch.from_numpy(GLYPHS.reshape(-1).copy()).cuda()
    base = words.data_ptr()
    _lib.call('cy_draw_boxes_u8', out.data_ptr(), packed.off.data_ptr(), packed.hw32.data_ptr(), packed.n, packed.nbytes,
              base, base + 4 * n, cols.data_ptr(), base + 20 * n, n, 2 * (64 + 48) + 119, glyphs.data_ptr(), base + 24 * n,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return draw.unpack_images(out, packed), int(words[-1].item())


def test_refused_boxes_draw_nothing():
    images = _canvas()
    packed = predict_fns.PackedImages(images)
    good = [(1, 1, 1, 7, 5, 42, draw.GREEN), (BIG, 5, 6, 20, 30, 9, BLUE)]
    bad_label = (BIG, 2, 2, 40, 40, 1000, draw.RED)               # would cover the good box's label if it were drawn
    bad_image = (len(SIZES), 0, 0, 5, 5, -1, draw.RED)
    for bad in (bad_label, bad_image, (-1, 0, 0, 5, 5, -1, draw.RED), (BIG, 2, 2, 40, 40, -2, draw.RED)):
        idx, xy, lab, col = _split(good + [bad])
        with pytest.raises(ValueError):
            draw.draw_boxes_device(packed, idx, xy, col, lab)
    out, bad = _raw_launch(packed, good + [bad_label, bad_image])
    assert bad == 2 and _same(out, _ref(images, good))
    out, bad = _raw_launch(packed, [bad_label, bad_image])
    assert bad == 2 and _same(out, images)
    out, bad = _raw_launch(packed, [good[1], good[0]])            # the image index descends: the second box is refused
    assert bad == 1 and _same(out, _ref(images, good[1:]))
    with pytest.raises(ValueError):
        draw.draw_boxes_device(packed, [0], np.array([[0.0, 0.0, np.nan, 1.0]]), draw.GREEN)
    assert torch.equal(packed.buf, torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).cuda())


def test_no_box_returns_a_copy():
    images = _canvas()
    packed = predict_fns.PackedImages(images)
    buf = draw.draw_boxes_device(packed, [], np.zeros((0, 4)), draw.GREEN)
    assert buf.data_ptr() != packed.buf.data_ptr() and torch.equal(buf, packed.buf)
    assert _same(draw.unpack_images(buf, packed), images)
    assert _same(draw.unpack_images(draw.draw_boxes_device(packed, [], np.zeros((0, 4)), draw.GREEN, np.zeros(0, np.int64)), packed), images)


# ------------------------------------------------------------------------------------------------ dark_pred / dark_class_pred
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


def _some_not_all(y0):
    """A confidence threshold halfway between two neighbouring confidences of the forward: some boxes pass, not all."""
    conf = np.unique(y0[..., 0::5])[::-1].astype(np.float64)
    assert len(conf) >= 8, 'the detector output has too few distinct confidences: %s' % conf
    return float(conf[5] + conf[6]) / 2


def _trunc(xy):
    return np.trunc(np.asarray(xy, dtype=np.float64)).astype(np.int64).reshape(-1, 4)


def test_dark_pred_draws_predictions_and_ground_truth(tmp_path):
    images = _images()
    dp, _, ddir, _ = _checkpoints(tmp_path)
    dark = models.DarkNet(dp).cuda()
    hw = np.array(IMAGE_HW)
    y0, none = predict_fns.dark_pred(images, dark, ddir, dp, 'last', batch_size=2)
    assert none is None
    conf_th = _some_not_all(y0)
    # ground truth whose values are float32 numbers: the device decodes float32 arrays, the restatement below this float64 one
    y = synth.gtsdb_labels(3, 2, 0, seed=41).astype(np.float32).astype(np.float64)
    y_hat, drawn = predict_fns.dark_pred(images, dark, ddir, dp, 'last', conf_th=conf_th, y=y, batch_size=2, draw=True)
    assert np.array_equal(y_hat, y0)
    _, _, idx, xy = predict_fns.dark_pred(images, dark, ddir, dp, 'last', is_end=False, conf_th=conf_th, batch_size=2)
    t_idx, t_xy, _ = utils_np.y_to_boxes_vec(y, 0, 64, hw, conf_th)
    print('conf_th %.6f: %d predicted boxes, %d ground-truth boxes' % (conf_th, len(idx), len(t_idx)))
    assert 4 <= len(idx) < 24 and len(t_idx) >= 3
    colors = np.array([draw.GREEN] * len(idx) + [draw.RED] * len(t_idx), dtype=np.uint8)
    ref = draw_ref(images, np.concatenate([idx, t_idx]), np.concatenate([_trunc(xy), _trunc(t_xy)]), colors, None, GLYPHS)
    assert _same(drawn, ref)
    only_pred = draw_ref(images, idx, _trunc(xy), colors[:len(idx)], None, GLYPHS)
    assert not _same(ref, only_pred)                                                            # the red pass shows
    _, drawn = predict_fns.dark_pred(images, dark, ddir, dp, 'last', conf_th=conf_th, batch_size=2, draw=True)
    assert _same(drawn, only_pred)
    y_hat, drawn = predict_fns.dark_pred(images, dark, ddir, dp, 'last', conf_th=2.0, batch_size=2, draw=True)
    assert np.array_equal(y_hat, y0) and _same(drawn, images)                                   # nothing over the threshold
    assert len(predict_fns.dark_pred(images, dark, ddir, dp, 'last', is_end=False, conf_th=conf_th, batch_size=2, draw=True)) == 4


def test_dark_pred_labels_with_the_detectors_classes(tmp_path):
    """A detector with a classifying head (darknet_r): predictions and ground truth carry their argmax class as the label."""
    images = _images()
    p = make_params(model='darknet_r', n_classes=43, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    torch.manual_seed(4)
    ddir = str(tmp_path / 'darknet_r')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.DarkNet(p).state_dict()}, False, ddir)
    dark = models.DarkNet(p).cuda()
    hw = np.array(IMAGE_HW)
    y0, _ = predict_fns.dark_pred(images, dark, ddir, p, 'last', batch_size=2)
    assert y0.shape == (3, 2, 2, 53)
    conf = np.unique(y0[..., 0:10:5])[::-1].astype(np.float64)
    assert len(conf) >= 8
    conf_th = float(conf[5] + conf[6]) / 2
    y = synth.gtsdb_labels(3, 2, 43, seed=42).astype(np.float32).astype(np.float64)
    y_hat, drawn = predict_fns.dark_pred(images, dark, ddir, p, 'last', conf_th=conf_th, y=y, batch_size=2, draw=True)
    assert np.array_equal(y_hat, y0)
    idx, xy, cls = utils_np.y_to_boxes_vec(y0, 43, 64, hw, conf_th)
    _, _, idx1, xy1 = predict_fns.dark_pred(images, dark, ddir, p, 'last', is_end=False, conf_th=conf_th, batch_size=2)
    t_idx, t_xy, t_cls = utils_np.y_to_boxes_vec(y, 43, 64, hw, conf_th)
    print('conf_th %.6f: %d predicted boxes (classes %s), %d ground-truth boxes (classes %s)' % (conf_th, len(idx), cls, len(t_idx), t_cls))
    assert 4 <= len(idx) < 24 and np.array_equal(idx, idx1) and len(t_idx) >= 3
    colors = np.array([draw.GREEN] * len(idx) + [draw.RED] * len(t_idx), dtype=np.uint8)
    ref = draw_ref(images, np.concatenate([idx, t_idx]), np.concatenate([_trunc(xy1), _trunc(t_xy)]), colors,
                   np.concatenate([cls, t_cls]), GLYPHS)
    assert _same(drawn, ref)
    assert not _same(ref, draw_ref(images, np.concatenate([idx, t_idx]), np.concatenate([_trunc(xy1), _trunc(t_xy)]), colors, None, GLYPHS))


def test_dark_class_pred_draws_the_classifiers_classes(tmp_path):
    images = _images()
    dp, cp, ddir, cdir = _checkpoints(tmp_path)
    dark, caps = models.DarkNet(dp).cuda(), models.CapsuleNet(cp).cuda()
    y0, _ = predict_fns.dark_pred(images, dark, ddir, dp, 'last', batch_size=2)
    conf_th = _some_not_all(y0)
    plain, none = predict_fns.dark_class_pred(images, dark, ddir, dp, caps, cdir, cp, 'last', batch_size=2, conf_th=conf_th)
    y_hat, drawn = predict_fns.dark_class_pred(images, dark, ddir, dp, caps, cdir, cp, 'last', batch_size=2, conf_th=conf_th, draw=True)
    assert none is None and y_hat.dtype == plain.dtype and np.array_equal(y_hat, plain)
    # the classifier's classes once more: the same crops (per chunk of 2 images) through the same forward (chunks of 2 crops)
    _, _, idx, xy = predict_fns.dark_pred(images, dark, ddir, dp, 'last', is_end=False, conf_th=conf_th, batch_size=2)
    crops = []
    for lo in (0, 2):
        packed = predict_fns.PackedImages(images[lo:lo + 2])
        mine = (idx >= lo) & (idx < lo + 2)
        rect = utils.crop_rectangles(xy[mine], idx[mine] - lo, packed.hw)
        crops.append(packed.crop_resize(idx[mine] - lo, rect, 32, 32, -128.0, 1.0 / 128.0, True))
    crops = torch.cat(crops, 0)
    caps.eval()
    with torch.no_grad():
        scores = torch.cat([caps(crops[lo:lo + 2]).data.reshape(-1, 43) for lo in range(0, len(idx), 2)], 0).cpu().numpy()
    classes = np.argmax(scores, axis=1)
    print('%d boxes, classes %s' % (len(idx), classes))
    assert 4 <= len(idx) < 24
    ref = draw_ref(images, idx, _trunc(xy), np.array([draw.GREEN] * len(idx), dtype=np.uint8), classes, GLYPHS)
    assert _same(drawn, ref)
    assert not _same(ref, draw_ref(images, idx, _trunc(xy), np.array([draw.GREEN] * len(idx), dtype=np.uint8), None, GLYPHS))
    y_none, drawn = predict_fns.dark_class_pred(images, dark, ddir, dp, caps, cdir, cp, 'last', batch_size=2, conf_th=2.0, draw=True)
    assert not y_none[..., 10:].any() and _same(drawn, images)


# ------------------------------------------------------------------------------------------------ detect_report
@pytest.mark.parametrize('seed,B,g,nb,C,strip', [(23, 2, 5, 2, 2, False),      # the class-agnostic shapes of the sweep's own tests
                                                 (24, 2, 12, 2, 3, False),
                                                 (23, 2, 5, 2, 2, True)])      # C = 0: arrays without class scores
def test_detect_report_equals_the_two_metrics(seed, B, g, nb, C, strip):
    y, y_hat = R.sweep_case(seed, B, g, nb, C, mark_frac=0.6 if g == 5 else 0.45)
    if strip:
        y, y_hat, C = np.ascontiguousarray(y[..., :5]), np.ascontiguousarray(y_hat[..., :5 * nb]), 0
    p = make_params(n_classes=C, darknet_input=416)
    out = metrics.detect_report(y, y_hat, p)
    ap, acc = metrics.detect_AP(y, y_hat, p), metrics.detect_acc(y, y_hat, p)
    print('detect_AP %.17g (%.17g), detect_acc %.17g (%.17g)' % (out['detect_AP'], ap, out['detect_acc'], acc))
    assert list(out) == ['detect_AP', 'detect_acc']
    assert out['detect_AP'] == ap and out['detect_acc'] == acc and 0.0 < ap <= 1.0 and 0.0 < acc <= 1.0


# ------------------------------------------------------------------------------------------------ main.py
def _main_module(tmp_path):
    _, _, ddir, cdir = _checkpoints(tmp_path)
    json.dump(dict(batch_size=4, n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, dropout=0.0),
              open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_detect', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m, ddir, cdir


def _six_images_in(folder):
    shapes = [im.shape for im in synth.raw_images(6)]
    assert sorted(os.listdir(folder)) == ['%d.ppm' % i for i in range(6)]
    return [read_ppm(os.path.join(folder, '%d.ppm' % i)) for i in range(6)], shapes


def test_main_detect_mode_writes_metrics_and_images(tmp_path):
    m, ddir, cdir = _main_module(tmp_path)
    out = m.main(['--mode', 'detect', '--model', 'darknet_d', '--synthetic', '6', '--model_dir', ddir, '--restore', 'last'])
    text = open(os.path.join(ddir, 'metric_output.txt')).read()
    fields = dict(f.split(':') for f in text.split(', ') if f)
    assert list(fields) == ['detect_AP', 'detect_acc'] == list(out)
    for k, v in fields.items():
        assert np.isfinite(float(v)) and float(v) == float(out[k]) and 0.0 <= float(v) <= 1.0
    written, shapes = _six_images_in(os.path.join(ddir, 'output'))
    assert [im.shape for im in written] == shapes
    # what was written: the ground truth in red over the synthetic images (and whatever the untrained detector found, in green)
    raw = synth.raw_images(6)
    assert any((im[(im != r).any(axis=2)] == np.array(draw.RED, np.uint8)).all(axis=1).any() for im, r in zip(written, raw))
    with pytest.raises(SystemExit):
        m.main(['--mode', 'detect', '--model', 'capsule', '--synthetic', '6', '--model_dir', cdir, '--restore', 'last'])
    with pytest.raises(SystemExit):
        m.main(['--mode', 'detect', '--model', 'darknet_d', '--synthetic', '6', '--model_dir', ddir])


def test_main_combined_branch_with_draw(tmp_path):
    m, ddir, _ = _main_module(tmp_path)
    argv = ['--mode', 'predict', '--model', 'darknet_d', '--combine', 'capsule', '--synthetic', '6', '--model_dir', ddir,
            '--restore', 'last']
    metric_file = os.path.join(ddir, 'combine-capsule_metric_output.txt')
    m.main(argv)
    plain = open(metric_file, 'rb').read()
    assert not os.path.exists(os.path.join(ddir, 'output'))                                     # without the flag nothing is drawn
    os.remove(metric_file)
    m.main(argv + ['--draw'])
    assert open(metric_file, 'rb').read() == plain
    written, shapes = _six_images_in(os.path.join(ddir, 'output'))
    assert [im.shape for im in written] == shapes

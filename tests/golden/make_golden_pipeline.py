#!/usr/bin/env python
"""Generate tests/golden/pipeline.npz by RUNNING THE REFERENCE (numpy / torch-CPU), like make_golden.py.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pipeline.py

Needs the reference checkout (CAPSYOLO_REFERENCE, found like make_golden.py finds it).  The fixture holds data only: the inputs and what
the reference's own metrics.detect_and_recog_mAP / detect_and_recog_acc / single_img_confusion / precision_and_recall /
average_precision and utils.y_to_boxes_vec / combine_y_hat returned for them.  About 12 s per mAP case and as much again for
its AP table.
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
import utils as ref_utils          # noqa: E402

C = 43
SIDE = 416


def map_case(seed, B, g, nb):
    """Ground truth: one box per marked cell (about 45 % of the cells), classes drawn from 3 labels.  Prediction: the ground
    truth jittered, confidence 0.35 .. 1 on object cells and 0 .. 0.6 elsewhere, class scores that favour the true class in
    about 70 % of the cells."""
    rng = np.random.default_rng(seed)
    labels = rng.choice(C, size=3, replace=False)
    mark = rng.random((B, g, g)) < 0.45
    y = np.zeros((B, g, g, 5 + C), dtype=np.float64)
    y[..., 0] = mark
    y[..., 1:3] = rng.random((B, g, g, 2)) * mark[..., None]
    y[..., 3:5] = (0.1 + 0.3 * rng.random((B, g, g, 2))) * mark[..., None]
    cls = labels[rng.integers(0, 3, (B, g, g))]
    y[..., 5:] = np.eye(C)[cls] * mark[..., None]
    h = np.zeros((B, g, g, 5 * nb + C), dtype=np.float32)
    for k in range(nb):
        jit = 1.0 + 0.3 * (rng.random((B, g, g, 4)) - 0.5)
        h[..., 5 * k + 1:5 * k + 5] = np.where(mark[..., None], y[..., 1:5] * jit,
                                               np.concatenate([rng.random((B, g, g, 2)), 0.05 + 0.3 * rng.random((B, g, g, 2))], -1))
        h[..., 5 * k] = np.where(mark, 0.35 + 0.65 * rng.random((B, g, g)), 0.6 * rng.random((B, g, g)))
    agree = rng.random((B, g, g)) < 0.7
    hcls = np.where(agree, cls, labels[rng.integers(0, 3, (B, g, g))])
    h[..., 5 * nb:] = 0.1 * rng.random((B, g, g, C)) + 0.8 * np.eye(C)[hcls]
    return y, h


def reference_ap_table(y, y_hat, p):
    """[43][10] from the reference's single_img_confusion, precision_and_recall and average_precision, with its decode."""
    iou_ths, conf_ths = np.linspace(0.5, 0.95, 10), np.linspace(0, 1, 100)
    decoded = [(ref_utils.y_to_boxes_vec(y, p, conf_th=th), ref_utils.y_to_boxes_vec(y_hat, p, conf_th=th)) for th in conf_ths]
    table = np.zeros((C, 10))
    for c in range(C):
        for i, iou_th in enumerate(iou_ths):
            ps, rs = [], []
            for (yi, yb, yc), (hi, hb, hc) in decoded:
                TP = FP = FN = 0
                for j in range(y.shape[0]):
                    tp, fp, fn = ref_metrics.single_img_confusion(yb[(yi == j) * (yc == c)], hb[(hi == j) * (hc == c)], iou_th)
                    TP, FP, FN = TP + tp, FP + fp, FN + fn
                pr, rc = ref_metrics.precision_and_recall(TP, FP, FN)
                ps.append(pr)
                rs.append(rc)
            table[c, i] = ref_metrics.average_precision(np.array(ps), np.array(rs))
    return table


def gen_map(arrays, tag, seed, B, g, nb):
    y, y_hat = map_case(seed, B, g, nb)
    p = SimpleNamespace(n_classes=C, darknet_input=SIDE, model='darknet_r')
    mAP = float(ref_metrics.detect_and_recog_mAP(y, y_hat, p))
    plt.close('all')
    f1 = float(ref_metrics.detect_and_recog_acc(y, y_hat, p))
    table = reference_ap_table(y, y_hat, p)
    present = int((np.sign(y[..., 5:].reshape(-1, C).sum(axis=0)) > 0).sum())
    distinct = len(np.unique(table))
    print('%s: mAP %.17g  f1 %.17g  classes present %d  distinct AP values %d' % (tag, mAP, f1, present, distinct))
    assert present >= 3 and 0.1 < mAP < 0.9 and distinct >= 5
    mask = np.sign(y[..., 5:].reshape(-1, C).sum(axis=0)) > 0
    assert np.mean(table[mask]) == mAP
    arrays.update({tag + '_y': y, tag + '_y_hat': y_hat, tag + '_mAP': np.float64(mAP), tag + '_f1': np.float64(f1),
                   tag + '_ap_table': table, tag + '_side': np.int64(SIDE)})


def gen_combine(arrays):
    rng = np.random.default_rng(77)
    B, g, nb, side = 4, 3, 2, 96
    image_hw = np.array([(80, 120), (96, 96), (100, 70), (64, 150)])
    dark = rng.random((B, g, g, 5 * nb)).astype(np.float32)
    dark[..., 3::5] = 0.05 + 0.4 * dark[..., 3::5]
    dark[..., 4::5] = 0.05 + 0.4 * dark[..., 4::5]
    p = SimpleNamespace(n_classes=0, darknet_input=side, n_grid=g)
    idx, xy, _ = ref_utils.y_to_boxes_vec(dark, p, image_hw=image_hw, conf_th=0.5)
    scores = rng.random((len(idx), C)).astype(np.float32)
    images = [np.zeros((h, w, 3), dtype=np.uint8) for h, w in image_hw]
    cells = []
    for i, index in enumerate(idx):
        cwh = ref_utils.xy_to_cwh(ref_utils.resize_box_xy(images[index].shape[0:2], (side, side), xy[i]))
        _, (row, col) = ref_utils.normalize_box_cwh((side, side), g, cwh)
        assert 0 <= row < g and 0 <= col < g
        cells.append((int(index), row, col))
    dup = len(cells) - len(set(cells))
    print('combine: %d boxes, %d in an already written cell' % (len(idx), dup))
    assert dup >= 3
    out = ref_utils.combine_y_hat(images, dark, scores, idx, xy, p)
    arrays.update({'combine_dark': dark, 'combine_image_hw': image_hw, 'combine_side': np.int64(side), 'combine_idx': idx,
                   'combine_xy': xy, 'combine_scores': scores, 'combine_y_hat': out})


if __name__ == '__main__':
    arrays = {}
    gen_map(arrays, 'map_a', 3, 3, 3, 2)
    gen_map(arrays, 'map_b', 4, 4, 4, 1)
    gen_combine(arrays)
    path = os.path.join(HERE, 'pipeline.npz')
    np.savez_compressed(path, **arrays)
    print('pipeline.npz %.1f KB' % (os.path.getsize(path) / 1024.0))

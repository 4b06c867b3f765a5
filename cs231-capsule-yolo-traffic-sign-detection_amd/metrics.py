"""Metrics of the reference on the device: metrics.detect_acc / detect_and_recog_acc / detect_AP /
detect_and_recog_mAP (metrics.py:193-339), detect_report (the two numbers of predict mode's detect-only branch from one sweep) and the classifier's report recog_auc / recog_pr (metrics.py:13-96).

The reference decodes both arrays to boxes with numpy and matches them with two nested Python loops per image
(metrics.py:136-147) every `eval_every` epochs; here the decoding (`cy_yolo_decode_boxes`) and the IoU matching
(`cy_detect_confusion`, one block per image) stay on the GPU and only TP / FP / FN come back.  `confusion_sweep` does the whole
confidence x IoU threshold sweep of the AP metrics with one decode per array and one launch (`cy_confusion_sweep`).

The reference computes recog_auc / recog_pr with sklearn's sort-based curves on the host.  Both are rank statistics of the N
positive scores, so here the device counts, for every row, the population elements at or above its positive score
(`cy_rank_counts`, no sort of the scores) and the host folds the integer counts into the two numbers.
"""
import numpy as np
import torch

from . import utils
from ._lib import call, query


def _confusion_of_boxes(gt, pr, y, y_hat, params, iou_th):
    (n1, gi, gxy, _), (n2, pi, pxy, _) = gt, pr
    batch = int(y.shape[0])
    g = int(y.shape[1])
    nb_max = max((int(y.shape[3]) - int(params.n_classes)) // 5, (int(y_hat.shape[3]) - int(params.n_classes)) // 5)
    out = torch.zeros(4, dtype=torch.int32, device='cuda')
    call('cy_detect_confusion', gi.data_ptr() if n1 else None, gxy.data_ptr() if n1 else None, n1,
         pi.data_ptr() if n2 else None, pxy.data_ptr() if n2 else None, n2, batch, float(iou_th), g * g * nb_max,
         out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    tp, fp, fn, bad = [int(v) for v in out.cpu().numpy()]
    if bad:
        raise AssertionError('malformed box (x1 > x2 or y1 > y2) in %d case(s)' % bad)
    return tp, fp, fn


def detect_confusion(y, y_hat, params, conf_th=0.5, iou_th=0.5):
    """(TP, FP, FN) summed over the batch; raises AssertionError on a malformed box like metrics.py:114-119."""
    return _confusion_of_boxes(utils.decode_boxes_device(y, params, None, conf_th),
                               utils.decode_boxes_device(y_hat, params, None, conf_th), y, y_hat, params, iou_th)


def precision_and_recall(tp, fp, fn):
    """metrics.py:150-160."""
    return (tp / (tp + fp) if tp + fp else 0.0), (tp / (tp + fn) if tp + fn else 0.0)


def detect_acc(y, y_hat, params):
    """metrics.py:245-262: F1 of the detector at confidence 0.5 / IoU 0.5."""
    p, r = precision_and_recall(*detect_confusion(y, y_hat, params))
    return 2 * p * r / (p + r + 1e-8)


def detect_and_recog_confusion(y, y_hat, params, conf_th=0.5, iou_th=0.5):
    """(TP, FP, FN) of metrics.py:264-280: the reference loops over classes and images and matches the boxes of one
    (image, class) pair at a time; here every pair is one block of the same kernel -- the boxes are sorted by the key
    image * n_classes + class on the device, which makes each pair a contiguous range."""
    C = int(params.n_classes)
    if C <= 0:
        raise ValueError('detect_and_recog_acc needs a classifying head (n_classes > 0)')
    sets = []
    for arr in (y, y_hat):
        n, idx, xy, cls = utils.decode_boxes_device(arr, params, None, conf_th)
        if n:
            key, order = torch.sort(idx.long() * C + cls.long(), stable=True)
            idx, xy = key.to(torch.int32).contiguous(), xy[order].contiguous()
        sets.append((n, idx, xy, cls))
    batch, g = int(y.shape[0]), int(y.shape[1])
    nb_max = max((int(y.shape[3]) - C) // 5, (int(y_hat.shape[3]) - C) // 5)
    (n1, gi, gxy, _), (n2, pi, pxy, _) = sets
    out = torch.zeros(4, dtype=torch.int32, device='cuda')
    call('cy_detect_confusion', gi.data_ptr() if n1 else None, gxy.data_ptr() if n1 else None, n1,
         pi.data_ptr() if n2 else None, pxy.data_ptr() if n2 else None, n2, batch * C, float(iou_th), g * g * nb_max,
         out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    tp, fp, fn, bad = [int(v) for v in out.cpu().numpy()]
    if bad:
        raise AssertionError('malformed box (x1 > x2 or y1 > y2) in %d case(s)' % bad)
    return tp, fp, fn


def detect_and_recog_acc(y, y_hat, params, show=False, save=False):
    """metrics.py:264-282: F1 of detection + recognition; the registry's metric of darknet_r and darkcapsule
    (main.py:262-264)."""
    p, r = precision_and_recall(*detect_and_recog_confusion(y, y_hat, params))
    return 2 * p * r / (p + r + 1e-8)


def recog_acc(y, y_hat, params):
    """metrics.py:9-11."""
    y, y_hat = [t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (y, y_hat)]
    return np.sum(y == np.argmax(y_hat, axis=1)) / len(y)


def recog_counts(y, y_hat, n_classes):
    """The rank counts of the classifier's report: (counts, correct) with counts int64 numpy [2][N][4] = (cnt_ge, cnt_gt, tp_ge,
    tp_gt) per row i -- the number of elements of a population, and of its positives, whose score is >= and > the row's positive
    score y_hat[i][y[i]]; counts[0]: micro (all N * C elements, positive iff column == label), counts[1]: per class (column y[i]) --
    and correct = np.sum(y == np.argmax(y_hat, axis=1)).  y [N] integer labels, y_hat [N][n_classes] scores, numpy arrays or
    device tensors.  Scores are compared as float32 VALUES (-0.0 == +0.0): another dtype is converted to float32 first, so
    float64 scores that differ only beyond float32 count as ties.  ValueError: no rows, a label outside 0..n_classes-1, a
    non-finite score (the reference stops on these too: sklearn refuses NaN / inf, np.eye(C)[y] a bad label)."""
    C = int(n_classes)
    s = _as_device_f32(y_hat)
    if s.dim() != 2 or int(s.shape[1]) != C or C < 1:
        raise ValueError('recog_counts: scores of shape %s for %d classes' % (tuple(s.shape), C))
    N = int(s.shape[0])
    lab = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y)
    if lab.is_floating_point() or lab.dtype == torch.bool or lab.dim() != 1 or int(lab.shape[0]) != N:
        raise ValueError('recog_counts: labels %s %s for %d rows of scores' % (lab.dtype, tuple(lab.shape), N))
    if N == 0:
        raise ValueError('recog_counts: no samples')
    lab = lab.to(device='cuda', dtype=torch.int64).contiguous()
    order = torch.sort(lab, stable=True)[1].to(torch.int32)               # rows grouped by label: the LABELS are sorted, never the scores
    ws = torch.empty(max(int(query('cy_rank_ws_ints', N, C)), 1), dtype=torch.int32, device='cuda')
    out = torch.zeros(8 * N + 2, dtype=torch.int32, device='cuda')        # the table, the number of correct rows, the error word
    call('cy_rank_counts', s.data_ptr(), lab.data_ptr(), order.data_ptr(), N, C, ws.data_ptr(), out.data_ptr(),
         out.data_ptr() + 4 * 8 * N, out.data_ptr() + 4 * (8 * N + 1), torch.cuda.current_stream().cuda_stream)
    host = out.cpu().numpy()
    if host[-1]:
        raise ValueError('recog_counts: %d label(s) outside 0..%d or non-finite score(s)' % (host[-1], C - 1))
    return host[:8 * N].astype(np.int64).reshape(2, N, 4), int(host[-2])


def auc_from_counts(cnt, n_pos, n_neg):
    """roc_curve + auc (trapezoid over the distinct thresholds) of a population with n_pos positives and n_neg negatives from
    the rows cnt [n_pos][4] of its positives: a positive beats the negatives below it and half of those it ties with.  The
    numerator is an integer (about 1.3e10 for the GTSRB test set: int64); NaN without a positive or without a negative."""
    if n_pos == 0 or n_neg == 0:
        return float('nan')
    neg_ge, neg_gt = cnt[:, 0] - cnt[:, 2], cnt[:, 1] - cnt[:, 3]
    return int(np.sum(2 * (n_neg - neg_ge) + (neg_ge - neg_gt), dtype=np.int64)) / (2 * int(n_pos) * int(n_neg))


def ap_from_counts(cnt, n_pos, n_neg):
    """average_precision_score (step-wise): every positive adds 1 / n_pos of recall at the precision of its threshold."""
    if n_pos == 0 or n_neg == 0:
        return float('nan')
    return float(np.sum(cnt[:, 2] / cnt[:, 0]) / n_pos)


def _per_class(fold, y, y_hat, n_classes):
    counts, _ = recog_counts(y, y_hat, n_classes)
    lab = (y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).astype(np.int64)
    out = np.full(int(n_classes), np.nan)
    for c in range(int(n_classes)):
        rows = counts[1][lab == c]
        out[c] = fold(rows, len(rows), len(lab) - len(rows))
    return out


def recog_auc_per_class(y, y_hat, n_classes):
    """[C] ROC AUC of every class against the rest (the roc_auc[i] the reference computes and drops, metrics.py:20-22); NaN for
    a class without a positive or without a negative."""
    return _per_class(auc_from_counts, y, y_hat, n_classes)


def recog_pr_per_class(y, y_hat, n_classes):
    """[C] average precision of every class (metrics.py:61-65); NaN for a class without a positive or without a negative."""
    return _per_class(ap_from_counts, y, y_hat, n_classes)


def recog_auc(y, y_hat, params, show=False, save=False, save_dir=None):
    """metrics.py:13-51 (the plot is out of scope: show / save are accepted and nothing is drawn): the micro-averaged ROC AUC
    over all N * C (sample, class) elements.  Scores are compared as float32, see recog_counts."""
    counts, _ = recog_counts(y, y_hat, params.n_classes)
    n = counts.shape[1]
    return auc_from_counts(counts[0], n, n * (int(params.n_classes) - 1))


def recog_pr(y, y_hat, params, show=False, save=False, save_dir=None):
    """metrics.py:54-96 (the plot is out of scope): the micro-averaged average precision.  Scores are compared as float32, see
    recog_counts."""
    counts, _ = recog_counts(y, y_hat, params.n_classes)
    return float(np.sum(counts[0][:, 2] / counts[0][:, 0]) / counts.shape[1])


def recog_report(y, y_hat, params):
    """What the class-only branch of predict mode reports (main.py:312-317), in its key order, from ONE count:
    {'recog_pr', 'recog_acc', 'recog_auc'}, each equal to what the function of that name returns."""
    counts, correct = recog_counts(y, y_hat, params.n_classes)
    n = counts.shape[1]
    return {'recog_pr': float(np.sum(counts[0][:, 2] / counts[0][:, 0]) / n), 'recog_acc': correct / n,
            'recog_auc': auc_from_counts(counts[0], n, n * (int(params.n_classes) - 1))}


def average_precision(p, r):
    """metrics.py:180-190: 11-point interpolated average precision."""
    out = []
    for level in np.linspace(0.0, 1.0, 11):
        args = np.argwhere(r >= level).flatten()
        out.append(max(p[args]) if len(args) else 0.0)
    return np.mean(out)


def detect_AP(y, y_hat, params, show=False, save=False, save_dir=None):
    """metrics.py:193-243 (plots are out of scope): boxes are decoded once per confidence threshold and matched on the
    device for each of the 10 IoU thresholds."""
    iou_ths, conf_ths = np.linspace(0.5, 0.95, 10), np.linspace(0, 1, 100)
    yt = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(device='cuda', dtype=torch.float32)
    ht = torch.as_tensor(np.asarray(y_hat) if not torch.is_tensor(y_hat) else y_hat).to(device='cuda', dtype=torch.float32)
    prec, rec = np.zeros((10, 100)), np.zeros((10, 100))
    for k, conf_th in enumerate(conf_ths):
        gt = utils.decode_boxes_device(yt, params, None, conf_th)
        pr = utils.decode_boxes_device(ht, params, None, conf_th)
        for i, iou_th in enumerate(iou_ths):
            prec[i, k], rec[i, k] = precision_and_recall(*_confusion_of_boxes(gt, pr, yt, ht, params, iou_th))
    return np.mean(np.array([average_precision(prec[i], rec[i]) for i in range(10)]))


def _as_device_f32(a):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device='cuda', dtype=torch.float32).contiguous()


def confusion_sweep_boxes(gt, pr, n_images, conf_ths, iou_ths, n_classes=0, max_per_group=None):
    """The sweep of confusion_sweep over two BOX LISTS instead of two label arrays: gt and pr are (image_indices [n], boxes_xy [n, 4] =
    (x1, y1, x2, y2), conf [n][, classes [n]]), arrays or tensors, both in the same pixels -- e.g. what utils.decode_boxes_device(...,
    with_conf=True) or predict_fns.dark_pred_tiled returned.  int64 numpy [K][n_classes or 1][T][3] = (TP, FP, FN) summed over the
    n_images images: a box counts at confidence threshold th iff (double)conf > th and is hit iff additionally a partner of its image
    (n_classes > 0: and of its class, which both lists must then carry) with IoU > iou_t that also counts exists (`cy_confusion_sweep`).
    max_per_group: boxes of one image (and class) the kernel has room for; default: the largest group of the two lists."""
    C = int(n_classes)
    conf_ths = np.ascontiguousarray(np.asarray(conf_ths, dtype=np.float64).reshape(-1))
    iou_ths = np.ascontiguousarray(np.asarray(iou_ths, dtype=np.float64).reshape(-1))
    K, T = len(conf_ths), len(iou_ths)
    if K < 1 or T < 1:
        raise ValueError('confusion_sweep needs at least one confidence and one IoU threshold')
    if int(n_images) < 1:
        raise ValueError('confusion_sweep_boxes: n_images must be >= 1, got %r' % (n_images,))
    Cn = C if C > 0 else 1

    def dev_t(a, dtype):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device='cuda', dtype=dtype).contiguous()
    sets = []
    for name, boxes in (('gt', gt), ('pr', pr)):
        if len(boxes) < (4 if C > 0 else 3) or (C > 0 and boxes[3] is None):
            raise ValueError('confusion_sweep_boxes: %s must be (image_indices, boxes_xy, conf%s)' % (name, ', classes' if C > 0 else ''))
        idx, xy, conf = dev_t(boxes[0], torch.int32).reshape(-1), dev_t(boxes[1], torch.float64).reshape(-1, 4), dev_t(boxes[2], torch.float32).reshape(-1)
        n = int(idx.numel())
        if int(xy.shape[0]) != n or int(conf.numel()) != n:
            raise ValueError('confusion_sweep_boxes: %s has %d image indices, %d boxes, %d confidences' % (name, n, xy.shape[0], conf.numel()))
        if n and C > 0:
            cls = dev_t(boxes[3], torch.int64).reshape(-1)
            key, order = torch.sort(idx.long() * C + cls, stable=True)
            idx, xy, conf = key.to(torch.int32).contiguous(), xy[order].contiguous(), conf[order].contiguous()
        sets.append((n, idx, xy, conf))
    (n1, gk, gxy, gcf), (n2, pk, pxy, pcf) = sets
    if max_per_group is None:
        max_per_group = max([1] + [int(torch.bincount(k.long()).max().item()) for n, k, _, _ in sets if n])
    ths = torch.from_numpy(np.concatenate([conf_ths, iou_ths])).cuda()
    out = torch.zeros(K * Cn * T * 3 + 1, dtype=torch.int32, device='cuda')          # the table, then the error word
    call('cy_confusion_sweep', gk.data_ptr() if n1 else None, gxy.data_ptr() if n1 else None, gcf.data_ptr() if n1 else None, n1,
         pk.data_ptr() if n2 else None, pxy.data_ptr() if n2 else None, pcf.data_ptr() if n2 else None, n2,
         int(n_images) * Cn, Cn, ths.data_ptr(), K, ths.data_ptr() + 8 * K, T, int(max_per_group),
         out.data_ptr(), out.data_ptr() + 4 * (K * Cn * T * 3), torch.cuda.current_stream().cuda_stream)
    host = out.cpu().numpy()
    if host[-1] >= 1 << 20:
        raise RuntimeError('confusion_sweep: a group holds more than %d boxes' % int(max_per_group))
    if host[-1]:
        raise AssertionError('malformed box (x1 > x2 or y1 > y2) in %d case(s)' % host[-1])
    return host[:-1].astype(np.int64).reshape(K, Cn, T, 3)


def confusion_sweep(y, y_hat, params, conf_ths, iou_ths, per_class=True):
    """(TP, FP, FN) of metrics.single_img_confusion summed over the images for EVERY confidence threshold, class and IoU
    threshold: int64 numpy [K][C or 1][T][3] (per_class=False: boxes are matched per image whatever their class, as in
    detect_AP).  The reference decodes both arrays again for every confidence threshold (metrics.py:298-302); a pair's IoU does
    not depend on it, so both are decoded once at min(conf_ths) with their confidences, sorted by image * C + class, and one
    launch counts everything: a box is hit at (th, iou_t) iff min(its confidence, best partner confidence at iou_t) > th.
    The counting is confusion_sweep_boxes on the two decoded lists."""
    C = int(params.n_classes)
    if per_class and C <= 0:
        raise ValueError('confusion_sweep(per_class=True) needs a classifying head (n_classes > 0)')
    conf_ths = np.ascontiguousarray(np.asarray(conf_ths, dtype=np.float64).reshape(-1))
    if len(conf_ths) < 1 or np.asarray(iou_ths).size < 1:
        raise ValueError('confusion_sweep needs at least one confidence and one IoU threshold')
    lo = np.float32(conf_ths.min())
    if float(lo) > conf_ths.min():          # the decode compares in float: never start above the lowest threshold
        lo = np.nextafter(lo, np.float32(-np.inf))
    yt, ht = _as_device_f32(y), _as_device_f32(y_hat)
    sets = []
    for arr in (yt, ht):
        n, idx, xy, cls, conf = utils.decode_boxes_device(arr, params, None, float(lo), with_conf=True)
        sets.append((idx, xy, conf, cls))
    batch, g = int(yt.shape[0]), int(yt.shape[1])
    nb_max = max((int(yt.shape[3]) - C) // 5, (int(ht.shape[3]) - C) // 5)
    return confusion_sweep_boxes(sets[0], sets[1], batch, conf_ths, iou_ths, C if per_class else 0, g * g * nb_max)


def _ap_table(counts):
    """[C][T] 11-point average precision over the K confidence thresholds of a count table [K][C][T][3]."""
    K, Cn, T, _ = counts.shape
    table = np.zeros((Cn, T))
    for c in range(Cn):
        for t in range(T):
            pr = [precision_and_recall(*[int(v) for v in counts[k, c, t]]) for k in range(K)]
            table[c, t] = average_precision(np.array([p for p, _ in pr]), np.array([r for _, r in pr]))
    return table


def detect_report(y, y_hat, params):
    """What the detect-only branch of predict mode reports (main.py:324-327), in its key order, from ONE sweep:
    {'detect_AP', 'detect_acc'}, each equal to what the function of that name returns (the same integer counts, folded the same
    way).  The class-agnostic count table over the 100 confidence thresholds of detect_AP plus detect_acc's 0.5, and the 10 IoU
    thresholds, whose first is detect_acc's 0.5: one decode per array and one launch where detect_AP decodes 200 times and
    launches 1000 times."""
    conf_ths, iou_ths = np.concatenate([np.linspace(0, 1, 100), [0.5]]), np.linspace(0.5, 0.95, 10)
    counts = confusion_sweep(y, y_hat, params, conf_ths, iou_ths, per_class=False)
    p, r = precision_and_recall(*[int(v) for v in counts[100, 0, 0]])
    return {'detect_AP': np.mean(_ap_table(counts[:100])[0]), 'detect_acc': 2 * p * r / (p + r + 1e-8)}


def detect_report_boxes(gt, pr, n_images):
    """detect_report for two box lists (image_indices, boxes_xy, conf) in the same pixels, e.g. the ground truth decoded with the
    images' sizes and the merged list of predict_fns.dark_pred_tiled: the same keys, thresholds and folding."""
    conf_ths, iou_ths = np.concatenate([np.linspace(0, 1, 100), [0.5]]), np.linspace(0.5, 0.95, 10)
    counts = confusion_sweep_boxes(gt, pr, n_images, conf_ths, iou_ths)
    p, r = precision_and_recall(*[int(v) for v in counts[100, 0, 0]])
    return {'detect_AP': np.mean(_ap_table(counts[:100])[0]), 'detect_acc': 2 * p * r / (p + r + 1e-8)}


def detect_and_recog_mAP(y, y_hat, params, show=False, save=False, save_dir=None):
    """metrics.py:284-339 (plots are out of scope): the mean, over the classes present in y and the 10 IoU thresholds, of the
    11-point AP over 100 confidence thresholds, boxes matched per image and class.  Sets params.n_classes = 43 like the
    reference (metrics.py:285)."""
    params.n_classes = 43
    counts = confusion_sweep(y, y_hat, params, np.linspace(0, 1, 100), np.linspace(0.5, 0.95, 10))
    avg_ps = _ap_table(counts)
    y_np = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    classes = np.sign(y_np[:, :, :, 5:].reshape(-1, 43).sum(axis=0))
    return np.mean(avg_ps[classes > 0])

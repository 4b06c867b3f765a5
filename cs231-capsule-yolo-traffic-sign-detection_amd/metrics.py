"""Detection metrics of the reference on the device: metrics.detect_acc / detect_and_recog_acc / detect_AP /
detect_and_recog_mAP (metrics.py:193-339).

The reference decodes both arrays to boxes with numpy and matches them with two nested Python loops per image
(metrics.py:136-147) every `eval_every` epochs; here the decoding (`cy_yolo_decode_boxes`) and the IoU matching
(`cy_detect_confusion`, one block per image) stay on the GPU and only TP / FP / FN come back.  `confusion_sweep` does the whole
confidence x IoU threshold sweep of the AP metrics with one decode per array and one launch (`cy_confusion_sweep`).
"""
import numpy as np
import torch

from . import utils
from ._lib import call


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


def confusion_sweep(y, y_hat, params, conf_ths, iou_ths, per_class=True):
    """(TP, FP, FN) of metrics.single_img_confusion summed over the images for EVERY confidence threshold, class and IoU
    threshold: int64 numpy [K][C or 1][T][3] (per_class=False: boxes are matched per image whatever their class, as in
    detect_AP).  The reference decodes both arrays again for every confidence threshold (metrics.py:298-302); a pair's IoU does
    not depend on it, so both are decoded once at min(conf_ths) with their confidences, sorted by image * C + class, and one
    launch counts everything: a box is hit at (th, iou_t) iff min(its confidence, best partner confidence at iou_t) > th."""
    C = int(params.n_classes)
    if per_class and C <= 0:
        raise ValueError('confusion_sweep(per_class=True) needs a classifying head (n_classes > 0)')
    conf_ths = np.ascontiguousarray(np.asarray(conf_ths, dtype=np.float64).reshape(-1))
    iou_ths = np.ascontiguousarray(np.asarray(iou_ths, dtype=np.float64).reshape(-1))
    K, T = len(conf_ths), len(iou_ths)
    if K < 1 or T < 1:
        raise ValueError('confusion_sweep needs at least one confidence and one IoU threshold')
    lo = np.float32(conf_ths.min())
    if float(lo) > conf_ths.min():          # the decode compares in float: never start above the lowest threshold
        lo = np.nextafter(lo, np.float32(-np.inf))
    yt, ht = _as_device_f32(y), _as_device_f32(y_hat)
    Cn = C if per_class else 1
    sets = []
    for arr in (yt, ht):
        n, idx, xy, cls, conf = utils.decode_boxes_device(arr, params, None, float(lo), with_conf=True)
        if n and per_class:
            key, order = torch.sort(idx.long() * C + cls.long(), stable=True)
            idx, xy, conf = key.to(torch.int32).contiguous(), xy[order].contiguous(), conf[order].contiguous()
        sets.append((n, idx, xy, conf))
    batch, g = int(yt.shape[0]), int(yt.shape[1])
    nb_max = max((int(yt.shape[3]) - C) // 5, (int(ht.shape[3]) - C) // 5)
    (n1, gk, gxy, gcf), (n2, pk, pxy, pcf) = sets
    ths = torch.from_numpy(np.concatenate([conf_ths, iou_ths])).cuda()
    out = torch.zeros(K * Cn * T * 3 + 1, dtype=torch.int32, device='cuda')          # the table, then the error word
    call('cy_confusion_sweep', gk.data_ptr() if n1 else None, gxy.data_ptr() if n1 else None, gcf.data_ptr() if n1 else None, n1,
         pk.data_ptr() if n2 else None, pxy.data_ptr() if n2 else None, pcf.data_ptr() if n2 else None, n2,
         batch * Cn, Cn, ths.data_ptr(), K, ths.data_ptr() + 8 * K, T, g * g * nb_max,
         out.data_ptr(), out.data_ptr() + 4 * (K * Cn * T * 3), torch.cuda.current_stream().cuda_stream)
    host = out.cpu().numpy()
    if host[-1] >= 1 << 20:
        raise RuntimeError('confusion_sweep: a group holds more than %d boxes' % (g * g * nb_max))
    if host[-1]:
        raise AssertionError('malformed box (x1 > x2 or y1 > y2) in %d case(s)' % host[-1])
    return host[:-1].astype(np.int64).reshape(K, Cn, T, 3)


def _ap_table(counts):
    """[C][T] 11-point average precision over the K confidence thresholds of a count table [K][C][T][3]."""
    K, Cn, T, _ = counts.shape
    table = np.zeros((Cn, T))
    for c in range(Cn):
        for t in range(T):
            pr = [precision_and_recall(*[int(v) for v in counts[k, c, t]]) for k in range(K)]
            table[c, t] = average_precision(np.array([p for p, _ in pr]), np.array([r for _, r in pr]))
    return table


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

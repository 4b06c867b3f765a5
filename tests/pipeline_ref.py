"""numpy restatements of the two-stage prediction chain -- TEST INFRASTRUCTURE ONLY (nothing in the product imports this).

The yardsticks of tests/test_gpu_pipeline.py on shapes that tests/golden/pipeline.npz does not hold; tests/test_pipeline_host.py
pins them against that fixture, which holds what the reference's own functions returned (tests/golden/make_golden_pipeline.py).

  confusion_sweep   metrics.detect_and_recog_mAP's loops (metrics.py:292-315) with ONE decode: a pair's IoU does not depend on the
                    confidence threshold, so box i is hit at (th, iou_t) iff min(conf_i, best partner conf at iou_t) > th
  combine_y_hat     utils.combine_y_hat (utils.py:336-351), vectorised; of several boxes in one cell the last one wins
  crop_rectangles   plot.py:22 (int() truncation of the corners) + clipping to the image
  crop_resize       cv2.resize(crop, (OW, OH)) with INTER_LINEAR's half-pixel convention, in float64 (no fixed-point rounding)
"""
import numpy as np

from oracle import utils_np


def decode_conf(y, n_classes, darknet_input, image_hw=None, conf_th=0.5):
    """utils_np.y_to_boxes_vec plus the stored confidence of every box (same order)."""
    idx, xy, cls = utils_np.y_to_boxes_vec(y, n_classes, darknet_input, image_hw, conf_th)
    batch, g, _, D = y.shape
    nb = int((D - n_classes) / 5)
    boxes = y[:, :, :, 0:5 * nb].reshape(batch, g, g, nb, 5)
    conf = boxes[boxes[:, :, :, :, 0] > conf_th, 0]
    return idx, xy, cls, conf


def iou_matrix(gt, pr):
    """metrics.calc_iou_individual (metrics.py:99-133) for every pair, the same operations in the same order."""
    if np.any(gt[:, 0] > gt[:, 2]) or np.any(gt[:, 1] > gt[:, 3]) or np.any(pr[:, 0] > pr[:, 2]) or np.any(pr[:, 1] > pr[:, 3]):
        raise AssertionError('malformed box')
    x1t, y1t, x2t, y2t = [gt[:, k][:, None] for k in range(4)]
    x1p, y1p, x2p, y2p = [pr[:, k][None, :] for k in range(4)]
    apart = (x2t < x1p) | (x2p < x1t) | (y2t < y1p) | (y2p < y1t)
    inter = (np.minimum(x2t, x2p) - np.maximum(x1t, x1p)) * (np.minimum(y2t, y2p) - np.maximum(y1t, y1p))
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / ((x2t - x1t) * (y2t - y1t) + (x2p - x1p) * (y2p - y1p) - inter)
    return np.where(apart, 0.0, iou)


def confusion_sweep(y, y_hat, n_classes, darknet_input, conf_ths, iou_ths, per_class=True):
    """int64 [K][C or 1][T][3]: (TP, FP, FN) summed over the images for every confidence threshold, class and IoU threshold."""
    conf_ths, iou_ths = np.asarray(conf_ths, dtype=np.float64), np.asarray(iou_ths, dtype=np.float64)
    K, T, B = len(conf_ths), len(iou_ths), y.shape[0]
    Cn = n_classes if per_class else 1
    lo = float(conf_ths.min())
    gi, gxy, gc, gcf = decode_conf(y, n_classes, darknet_input, None, lo)
    pi, pxy, pc, pcf = decode_conf(y_hat, n_classes, darknet_input, None, lo)
    gkey = gi * Cn + gc if per_class else gi
    pkey = pi * Cn + pc if per_class else pi
    out = np.zeros((K, Cn, T, 3), dtype=np.int64)
    for grp in np.union1d(gkey, pkey):
        G, P = gxy[gkey == grp], pxy[pkey == grp]
        gconf, pconf = gcf[gkey == grp].astype(np.float64), pcf[pkey == grp].astype(np.float64)
        iou = iou_matrix(G, P)                                                   # [n1][n2]
        over = iou[:, :, None] > iou_ths[None, None, :]                          # [n1][n2][T]
        gbest = np.where(over, pconf[None, :, None], -np.inf).max(axis=1, initial=-np.inf)     # [n1][T]
        pbest = np.where(over, gconf[:, None, None], -np.inf).max(axis=0, initial=-np.inf)     # [n2][T]
        n1 = (gconf[None, :] > conf_ths[:, None]).sum(1)                         # [K]
        n2 = (pconf[None, :] > conf_ths[:, None]).sum(1)
        gh = (np.minimum(gconf[:, None], gbest)[None] > conf_ths[:, None, None]).sum(1)        # [K][T]
        ph = (np.minimum(pconf[:, None], pbest)[None] > conf_ths[:, None, None]).sum(1)
        c = int(grp) % Cn
        out[:, c, :, 0] += gh
        out[:, c, :, 1] += n2[:, None] - ph
        out[:, c, :, 2] += n1[:, None] - gh
    return out


def ap_table(counts):
    """[C][T] average precision from a count table [K][C][T][3] (metrics.py:313-317)."""
    K, C, T, _ = counts.shape
    table = np.zeros((C, T))
    for c in range(C):
        for t in range(T):
            p, r = np.zeros(K), np.zeros(K)
            for k in range(K):
                tp, fp, fn = [int(v) for v in counts[k, c, t]]
                p[k] = tp / (tp + fp) if tp + fp else 0.0
                r[k] = tp / (tp + fn) if tp + fn else 0.0
            table[c, t] = utils_np.average_precision(p, r)
    return table


MAP_CONF_THS, MAP_IOU_THS = np.linspace(0, 1, 100), np.linspace(0.5, 0.95, 10)


def detect_and_recog_mAP(y, y_hat, darknet_input):
    """metrics.py:284-339 without the plots: (mAP, AP table [43][10])."""
    table = ap_table(confusion_sweep(y, y_hat, 43, darknet_input, MAP_CONF_THS, MAP_IOU_THS))
    mask = np.sign(y[:, :, :, 5:].reshape(-1, 43).sum(axis=0)) > 0
    return np.mean(table[mask]), table


def box_cells(image_hw, image_indices, boxes_xy, side, n_grid):
    """(row, col) of every box: resize_box_xy -> xy_to_cwh -> normalize_box_cwh (utils.py:198-230), int() = truncation."""
    hw = np.asarray(image_hw, dtype=np.float64).reshape(-1, 2)[image_indices]
    w_ratio, h_ratio = 1. * side / hw[:, 1], 1. * side / hw[:, 0]
    xc = (boxes_xy[:, 0] * w_ratio + boxes_xy[:, 2] * w_ratio) / 2
    yc = (boxes_xy[:, 1] * h_ratio + boxes_xy[:, 3] * h_ratio) / 2
    grid = 1. * side / n_grid
    return np.trunc(yc / grid).astype(np.int64), np.trunc(xc / grid).astype(np.int64)


def combine_y_hat(image_hw, dark_y_hat, class_y_hat, image_indices, boxes_xy, side, n_grid):
    """utils.py:336-351: float64 [B][g][g][D + C]; raises ValueError for a box outside the grid (the reference raises
    IndexError or wraps around)."""
    B, g, _, D = dark_y_hat.shape
    C = class_y_hat.shape[1]
    y_hat = np.zeros((B, g, g, D + C))
    y_hat[..., :D] = dark_y_hat
    if len(image_indices):
        row, col = box_cells(image_hw, image_indices, boxes_xy, side, n_grid)
        if np.any((row < 0) | (row >= g) | (col < 0) | (col >= g)):
            raise ValueError('box centre outside the grid')
        cell = (np.asarray(image_indices) * g + row) * g + col
        last = {}
        for i, c in enumerate(cell):                      # the last box of a cell wins
            last[int(c)] = i
        flat = y_hat.reshape(B * g * g, D + C)
        for c, i in last.items():
            flat[c, D:] = class_y_hat[i]
    return y_hat


def crop_rectangles(boxes_xy, image_indices, image_hw):
    """int64 [n][4] = (y0, y1, x0, x1), half-open: the corners truncated like int() (plot.py:22), then clipped to
    [0, w] x [0, h] (Python's wrap-around of negative indices is not kept).  ValueError on an empty rectangle."""
    hw = np.asarray(image_hw, dtype=np.int64).reshape(-1, 2)[image_indices]
    t = np.trunc(np.asarray(boxes_xy, dtype=np.float64)).astype(np.int64)
    x0, x1 = np.clip(t[:, 0], 0, hw[:, 1]), np.clip(t[:, 2], 0, hw[:, 1])
    y0, y1 = np.clip(t[:, 1], 0, hw[:, 0]), np.clip(t[:, 3], 0, hw[:, 0])
    rect = np.stack([y0, y1, x0, x1], axis=1)
    if np.any((y1 <= y0) | (x1 <= x0)):
        raise ValueError('empty crop')
    return rect


def crop_resize(image, rect, OH, OW, shift=0.0, scale=1.0):
    """float64 [OH][OW][3]: the crop resized as a stand-alone image, bilinear with half-pixel centres, then (v + shift) * scale."""
    y0, y1, x0, x1 = [int(v) for v in rect]
    crop = np.asarray(image)[y0:y1, x0:x1].astype(np.float64)
    ch, cw = crop.shape[:2]

    def taps(n_out, n_in):
        s = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
        r0 = np.floor(s)
        return np.clip(r0, 0, n_in - 1).astype(int), np.clip(r0 + 1, 0, n_in - 1).astype(int), s - r0
    ra, rb, fy = taps(OH, ch)
    ca, cb, fx = taps(OW, cw)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = crop[ra][:, ca] + fx * (crop[ra][:, cb] - crop[ra][:, ca])
    bot = crop[rb][:, ca] + fx * (crop[rb][:, cb] - crop[rb][:, ca])
    return (top + fy * (bot - top) + shift) * scale


def sweep_case(seed, B, g, nb, C, mark_frac=0.45, n_labels=3):
    """A seeded (y float64 [B,g,g,5+C], y_hat float32 [B,g,g,5 nb+C]) pair: ground truth on about mark_frac of the cells with
    classes from n_labels labels; predictions that are the ground truth jittered on those cells and random boxes elsewhere."""
    rng = np.random.default_rng(seed)
    labels = rng.choice(C, size=min(n_labels, C), replace=False)
    mark = rng.random((B, g, g)) < mark_frac
    y = np.zeros((B, g, g, 5 + C), dtype=np.float64)
    y[..., 0] = mark
    y[..., 1:3] = rng.random((B, g, g, 2)) * mark[..., None]
    y[..., 3:5] = (0.1 + 0.3 * rng.random((B, g, g, 2))) * mark[..., None]
    cls = labels[rng.integers(0, len(labels), (B, g, g))]
    y[..., 5:] = np.eye(C)[cls] * mark[..., None]
    h = np.zeros((B, g, g, 5 * nb + C), dtype=np.float32)
    for k in range(nb):
        jit = 1.0 + 0.3 * (rng.random((B, g, g, 4)) - 0.5)
        other = np.concatenate([rng.random((B, g, g, 2)), 0.05 + 0.3 * rng.random((B, g, g, 2))], -1)
        h[..., 5 * k + 1:5 * k + 5] = np.where(mark[..., None], y[..., 1:5] * jit, other)
        h[..., 5 * k] = np.where(mark, 0.35 + 0.65 * rng.random((B, g, g)), 0.6 * rng.random((B, g, g)))
    hcls = np.where(rng.random((B, g, g)) < 0.7, cls, labels[rng.integers(0, len(labels), (B, g, g))])
    h[..., 5 * nb:] = 0.1 * rng.random((B, g, g, C)) + 0.8 * np.eye(C)[hcls]
    return y, h

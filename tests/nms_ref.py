"""numpy restatement of the suppression step (csrc/nms.hip, `cy_nms_boxes`) -- TEST INFRASTRUCTURE ONLY (nothing in the product
imports this).  Plain loops, one pair at a time, in float64 with the operations of metrics.calc_iou_individual in its order.

  box_iou    the IoU of one pair with the early-out (0.0 for boxes that lie apart)
  malformed  a corner that is not finite, x1 > x2 or y1 > y2
  nms        keep mask in list order, the survivors' list indices in output order, and `visited`: the IoU of every pair the greedy
             sweep compared (the tests' precondition that no decision sits on the threshold reads it)
  outputs    the K output slots and the count as the kernel writes them
  generators the lists of the tests (the host tests check the restatement on them, the GPU tests the kernel)
"""
import numpy as np


def box_iou(a, p):
    x1t, y1t, x2t, y2t = (np.float64(v) for v in a)
    x1p, y1p, x2p, y2p = (np.float64(v) for v in p)
    if x2t < x1p or x2p < x1t or y2t < y1p or y2p < y1t:
        return np.float64(0.0)
    inter = (min(x2t, x2p) - max(x1t, x1p)) * (min(y2t, y2p) - max(y1t, y1p))
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / ((x2t - x1t) * (y2t - y1t) + (x2p - x1p) * (y2p - y1p) - inter)


def malformed(b):
    return bool(not np.all(np.isfinite(b)) or b[0] > b[2] or b[1] > b[3])


def nms(box_img, box_xy, conf, cls=None, n_images=None, iou_th=0.45, class_aware=False, per_image=0, max_per_image=None):
    """(keep uint8-like int32 [n], order int64 [survivors], visited float64 [pairs], overflow: images over max_per_image)."""
    img = np.asarray(box_img, dtype=np.int64).reshape(-1)
    xy = np.asarray(box_xy, dtype=np.float64).reshape(-1, 4)
    conf = np.asarray(conf, dtype=np.float32).reshape(-1)
    n = len(img)
    if n_images is None:
        n_images = int(img.max()) + 1 if n else 1
    keep = np.zeros(n, dtype=np.int32)
    order, visited, overflow = [], [], 0
    for b in range(n_images):
        mine = np.flatnonzero(img == b)
        if max_per_image is not None and len(mine) > max_per_image:
            overflow += 1
            continue
        with np.errstate(invalid='ignore'):
            visit = mine[np.argsort(-conf[mine], kind='stable')]        # descending, ties to the lower index, NaN last
        kept = []
        for i in visit:
            if per_image and len(kept) == per_image:
                break
            hit = False
            if not malformed(xy[i]):
                for k in kept:
                    if malformed(xy[k]) or (class_aware and cls[k] != cls[i]):
                        continue
                    iou = box_iou(xy[k], xy[i])
                    visited.append(iou)
                    if iou > iou_th:                                     # (False for a NaN)
                        hit = True
                        break
            if not hit:
                kept.append(i)
        keep[kept] = 1
        order.extend(kept)
    return keep, np.asarray(order, dtype=np.int64), np.asarray(visited, dtype=np.float64), overflow


def outputs(order, box_img, box_xy, conf, cls, K):
    """(count, out_img int32 [K], out_xy float64 [K, 4], out_conf float32 [K], out_cls int32 [K] | None, out_src int32 [K])."""
    s = order[:K]
    out_img, out_src = np.zeros(K, np.int32), np.zeros(K, np.int32)
    out_xy, out_conf = np.zeros((K, 4), np.float64), np.zeros(K, np.float32)
    out_img[:len(s)] = np.asarray(box_img)[s]
    out_xy[:len(s)] = np.asarray(box_xy, dtype=np.float64).reshape(-1, 4)[s]
    out_conf[:len(s)] = np.asarray(conf, dtype=np.float32)[s]
    out_src[:len(s)] = s
    out_cls = None
    if cls is not None:
        out_cls = np.zeros(K, np.int32)
        out_cls[:len(s)] = np.asarray(cls)[s]
    return len(order), out_img, out_xy, out_conf, out_cls, out_src


# ------------------------------------------------------------------------------------------------ the lists of the tests
def known_answers():
    """name -> (kwargs of nms, expected keep).  Every list is (box_img, box_xy, conf, cls)."""
    nested = [[0, 0, 10, 10], [1, 1, 9, 9], [2, 2, 8, 8]]                # IoU 0.64 (0-1), 0.36 (0-2), 0.5625 (1-2)
    cases = {}
    cases['nested'] = (dict(box_img=[0, 0, 0], box_xy=nested, conf=[0.7, 0.9, 0.8], iou_th=0.45), [0, 1, 0])
    cases['nested_loose'] = (dict(box_img=[0, 0, 0], box_xy=nested, conf=[0.9, 0.7, 0.8], iou_th=0.6), [1, 0, 1])
    cases['ties'] = (dict(box_img=[0, 0, 0], box_xy=[[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]], conf=[0.5, 0.5, 0.5], iou_th=0.45),
                     [1, 0, 1])
    # inter 3 x 3 = 9, union 9 + 20 - 9 = 20: the IoU is the double 0.45 itself, and the comparison is strict
    cases['on_threshold'] = (dict(box_img=[0, 0], box_xy=[[0, 0, 3, 3], [0, 0, 4, 5]], conf=[0.9, 0.8], iou_th=0.45), [1, 1])
    cases['below_threshold'] = (dict(box_img=[0, 0], box_xy=[[0, 0, 3, 3], [0, 0, 4, 5]], conf=[0.9, 0.8], iou_th=0.44), [1, 0])
    cases['touching'] = (dict(box_img=[0, 0, 0], box_xy=[[0, 0, 5, 5], [5, 0, 10, 5], [5, 5, 10, 10]], conf=[0.9, 0.8, 0.7], iou_th=0.0),
                         [1, 1, 1])
    same = [[0, 0, 10, 10], [0, 0, 10, 9], [0, 0, 10, 8]]
    cases['class_agnostic'] = (dict(box_img=[0, 0, 0], box_xy=same, conf=[0.9, 0.8, 0.7], cls=[1, 2, 1], iou_th=0.45), [1, 0, 0])
    cases['class_aware'] = (dict(box_img=[0, 0, 0], box_xy=same, conf=[0.9, 0.8, 0.7], cls=[1, 2, 1], iou_th=0.45, class_aware=True),
                            [1, 1, 0])
    far = [[0, 0, 4, 4], [10, 0, 14, 4], [20, 0, 24, 4], [30, 0, 34, 4]]
    cases['per_image'] = (dict(box_img=[0, 0, 0, 0], box_xy=far, conf=[0.6, 0.9, 0.7, 0.8], iou_th=0.45, per_image=2), [0, 1, 0, 1])
    # images do not interact (the same box in images 0 and 2), image 1 has no box
    cases['two_images'] = (dict(box_img=[0, 0, 2, 2], box_xy=[[0, 0, 10, 10], [1, 1, 9, 9], [0, 0, 10, 10], [1, 1, 9, 9]],
                                conf=[0.9, 0.8, 0.7, 0.95], n_images=3, iou_th=0.45), [1, 0, 0, 1])
    # an inverted box and a NaN corner pass through and suppress nothing, although they come first
    cases['malformed'] = (dict(box_img=[0, 0, 0, 0], box_xy=[[10, 0, 0, 10], [0, 0, 10, 10], [0, np.nan, 10, 10], [0, 0, 10, 9]],
                               conf=[0.99, 0.9, 0.95, 0.8], iou_th=0.45), [1, 1, 1, 0])
    return cases


def integer_lists(counts, seed, n_classes=3):
    """Boxes with integer corners in [0, 64): every IoU is an exact rational below 2^53, so the decisions do not depend on the
    arithmetic.  counts: boxes per image (0 allowed); confidence ties are planted."""
    rng = np.random.RandomState(seed)
    img = np.concatenate([np.full(c, b, dtype=np.int32) for b, c in enumerate(counts)])
    n = len(img)
    a, b = rng.randint(0, 64, (n, 2)), rng.randint(0, 64, (n, 2))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    xy = np.concatenate([lo, hi], axis=1).astype(np.float64)           # x1, y1, x2, y2 (a box may be a line or a point)
    conf = (rng.randint(1, 200, n) / 200.0).astype(np.float32)          # 199 values for hundreds of boxes: many ties
    cls = rng.randint(0, n_classes, n).astype(np.int32)
    return img, xy, conf, cls


def float_lists(seed, n=400, n_images=3, n_classes=3):
    """Boxes around clustered centres (60 per image, spread 8 pixels), so that roughly a quarter of them is suppressed at IoU 0.45."""
    rng = np.random.RandomState(seed)
    img = np.sort(rng.randint(0, n_images, n)).astype(np.int32)
    centres = rng.uniform(40.0, 560.0, (n_images, 60, 2))
    which = rng.randint(0, 60, n)
    c = centres[img, which] + rng.normal(0.0, 8.0, (n, 2))
    wh = rng.uniform(20.0, 40.0, (n, 2))
    xy = np.concatenate([c - wh / 2, c + wh / 2], axis=1)
    conf = rng.uniform(0.01, 1.0, n).astype(np.float32)
    cls = rng.randint(0, n_classes, n).astype(np.int32)
    return img, xy, conf, cls


def y_hat_case():
    """The detector output of the nms_y_hat tests: n = 2, g = 4, n_boxes = 2, C = 3, with neighbouring cells firing on the same sign, a
    negative and a NaN confidence."""
    rng = np.random.RandomState(7)
    n, g, nb, C = 2, 4, 2, 3
    y = np.zeros((n, g, g, 5 * nb + C), dtype=np.float32)
    y[..., 0:5 * nb:5] = rng.uniform(0.05, 1.0, (n, g, g, nb))
    y[..., 1:5 * nb:5] = rng.uniform(0.3, 0.7, (n, g, g, nb))
    y[..., 2:5 * nb:5] = rng.uniform(0.3, 0.7, (n, g, g, nb))
    y[..., 3:5 * nb:5] = rng.uniform(0.6, 0.9, (n, g, g, nb))          # a box spans several cells: neighbours overlap
    y[..., 4:5 * nb:5] = rng.uniform(0.6, 0.9, (n, g, g, nb))
    y[..., 5 * nb:] = rng.uniform(0.0, 1.0, (n, g, g, C))
    y[0, 1, 2, 0] = -0.25
    y[1, 3, 0, 5] = np.nan
    y[0, 0, 0, 5] = 0.0
    return y, dict(n_grid=g, n_boxes=nb, n_classes=C, darknet_input=64)

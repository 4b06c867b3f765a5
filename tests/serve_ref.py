"""numpy restatements behind the streaming detector's two kernels (csrc/serve.hip): the rectangle rule with the bad-box policy
(utils.crop_rectangles without the raise) and the record packing (arg-max + gather).  The crop pixels are not restated: they are
compared with the existing crop kernel."""
import numpy as np

HEADER_DTYPE = np.dtype([('total', '<i4'), ('kept', '<i4'), ('crop_err', '<i4'), ('resize_err', '<i4')])
RECORD_DTYPE = np.dtype([('xy', '<f8', (4,)), ('image', '<i4'), ('cls', '<i4'), ('conf', '<f4'), ('score', '<f4')])


def slot_rectangles(count, box_img, box_xy, image_hw, K):
    """(rect int64 [K, 4] = (y0, y1, x0, x1), bad bool [K], live bool [K]).  Slot s is live iff s < min(count, K); a live slot is
    bad when a corner is not finite, its image index lies outside the images or its rectangle is empty after clipping.  Bad and
    dead slots have the rectangle (0, 0, 0, 0)."""
    hw = np.asarray(image_hw, dtype=np.int64).reshape(-1, 2)
    xy = np.asarray(box_xy, dtype=np.float64).reshape(-1, 4)
    idx = np.asarray(box_img, dtype=np.int64).reshape(-1)
    rect = np.zeros((K, 4), dtype=np.int64)
    bad, live = np.zeros(K, dtype=bool), np.zeros(K, dtype=bool)
    for s in range(min(int(count), K)):
        live[s] = True
        if not (0 <= idx[s] < len(hw)) or not np.all(np.isfinite(xy[s])):
            bad[s] = True
            continue
        h, w = float(hw[idx[s], 0]), float(hw[idx[s], 1])
        t = np.trunc(xy[s])
        x0, x1 = np.clip(t[0], 0, w), np.clip(t[2], 0, w)
        y0, y1 = np.clip(t[1], 0, h), np.clip(t[3], 0, h)
        r = np.array([y0, y1, x0, x1]).astype(np.int64)
        if r[1] <= r[0] or r[3] <= r[2]:
            bad[s] = True
            continue
        rect[s] = r
    return rect, bad, live


def pack(scores, count, box_img, box_xy, conf, rect, crop_err, resize_err, K):
    """The record buffer as bytes (uint8 [16 + 48 K]): header, then per slot the gathered box, np.argmax of its scores and that
    score; class -1 and score 0 for a slot with a zero rectangle; zeros and class -1 behind min(count, K)."""
    scores = np.asarray(scores, dtype=np.float32).reshape(K, -1)
    rect = np.asarray(rect).reshape(K, 4)
    head = np.zeros(1, dtype=HEADER_DTYPE)
    kept = min(max(int(count), 0), K)
    head[0] = (int(count), kept, int(crop_err), int(resize_err))
    rec = np.zeros(K, dtype=RECORD_DTYPE)
    rec['cls'] = -1
    for s in range(kept):
        rec['xy'][s] = np.asarray(box_xy, dtype=np.float64).reshape(-1, 4)[s]
        rec['image'][s] = int(np.asarray(box_img).reshape(-1)[s])
        rec['conf'][s] = np.asarray(conf, dtype=np.float32).reshape(-1)[s]
        if rect[s].any():
            c = int(np.argmax(scores[s]))
            rec['cls'][s], rec['score'][s] = c, scores[s, c]
    return np.concatenate([head.view(np.uint8), rec.view(np.uint8)])

"""numpy restatement (float64, the operation order of include/capsyolo_hip.h) of the tiled decode `cy_yolo_decode_tiles_conf`, and of
the threshold sweep over box lists that metrics.confusion_sweep_boxes runs on the device.  Loops, not vectors: small cases only."""
import numpy as np

SIDES = ('left', 'right', 'top', 'bottom')


def tile_ok(frame, rect, frame_hw):
    if not (0 <= frame < len(frame_hw)):
        return False
    H, W = (int(v) for v in frame_hw[frame])
    y0, y1, x0, x1 = (int(v) for v in rect)
    return 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W


def border_sides(box, rect, H, W, margin):
    """Which of the four sides of the border rule fire for a box in tile pixels (none when margin < 0; a NaN corner fires none)."""
    bx1, by1, bx2, by2 = (np.float64(v) for v in box)
    y0, y1, x0, x1 = (int(v) for v in rect)
    th, tw = np.float64(y1 - y0), np.float64(x1 - x0)
    m = np.float64(margin)
    if m < 0:
        return (False, False, False, False)
    return (bool(x0 > 0 and bx1 < m), bool(x1 < W and bx2 > tw - m), bool(y0 > 0 and by1 < m), bool(y1 < H and by2 > th - m))


def decode_tiles(y, n_classes, tile_frame, tile_rect, frame_hw, conf_th, margin):
    """dict(count, dropped, err, idx int32, xy float64 [count, 4], cls int32 | None, conf float32, tile int32, fired: how often each
    side of the border rule fired) for y float32 [Bt, g, g, 5 nb + C]: every kept box, in (tile, row, column, box) order."""
    y = np.asarray(y, dtype=np.float32)
    Bt, g, _, D = y.shape
    C = int(n_classes)
    nb = (D - C) // 5
    tile_frame = np.asarray(tile_frame).reshape(-1)
    tile_rect = np.asarray(tile_rect).reshape(-1, 4)
    frame_hw = np.asarray(frame_hw).reshape(-1, 2)
    th_ = np.float32(conf_th)
    idx, xy, cls, conf, tile = [], [], [], [], []
    dropped, err, fired = 0, 0, dict.fromkeys(SIDES, 0)
    for b in range(Bt):
        frame = int(tile_frame[b])
        if not tile_ok(frame, tile_rect[b], frame_hw):
            err += 1
            continue
        H, W = (int(v) for v in frame_hw[frame])
        y0, y1, x0, x1 = (int(v) for v in tile_rect[b])
        ih, iw = np.float64(y1 - y0), np.float64(x1 - x0)
        gw, gh = 1.0 * iw / g, 1.0 * ih / g
        for row in range(g):
            for col in range(g):
                cell = y[b, row, col]
                for k in range(nb):
                    cf = cell[5 * k]
                    if not cf > th_:
                        continue
                    with np.errstate(all='ignore'):
                        xc, yc = np.float64(cell[5 * k + 1]) * gw, np.float64(cell[5 * k + 2]) * gh
                        w_, h_ = np.float64(cell[5 * k + 3]) * iw, np.float64(cell[5 * k + 4]) * ih
                        xc, yc = xc + col * gw, yc + row * gh
                        box = (xc - w_ / 2, yc - h_ / 2, xc + w_ / 2, yc + h_ / 2)
                    sides = border_sides(box, tile_rect[b], H, W, margin)
                    if any(sides):
                        dropped += 1
                        for name, hit in zip(SIDES, sides):
                            fired[name] += int(hit)
                        continue
                    idx.append(frame)
                    xy.append([box[0] + np.float64(x0), box[1] + np.float64(y0), box[2] + np.float64(x0), box[3] + np.float64(y0)])
                    conf.append(cf)
                    tile.append(b)
                    if C:
                        cls.append(_first_max(cell[5 * nb:]))
    return dict(count=len(idx), dropped=dropped, err=err, idx=np.array(idx, dtype=np.int32),
                xy=np.array(xy, dtype=np.float64).reshape(-1, 4), cls=np.array(cls, dtype=np.int32) if C else None,
                conf=np.array(conf, dtype=np.float32), tile=np.array(tile, dtype=np.int32), fired=fired)


def _first_max(v):
    """The decode kernels' arg-max: the first maximum wins, and a NaN never beats what stands (`v > best` is false)."""
    best = 0
    for c in range(1, len(v)):
        if v[c] > v[best]:
            best = c
    return best


def box_iou(a, b):
    """csrc/box_iou.h in float64, as tests/nms_ref.py restates it."""
    import nms_ref
    return nms_ref.box_iou(a, b)


def confusion_sweep(gt, pr, n_images, conf_ths, iou_ths):
    """int64 [K, T, 3] = (TP, FP, FN) of the class-agnostic sweep over box lists gt / pr = (idx, xy, conf): a box counts at threshold th
    iff float64(conf) > th and is hit iff a partner of its image with IoU > iou_t that also counts exists (include/capsyolo_hip.h,
    cy_confusion_sweep)."""
    g_idx, g_xy, g_cf = (np.asarray(a) for a in gt[:3])
    p_idx, p_xy, p_cf = (np.asarray(a) for a in pr[:3])
    out = np.zeros((len(conf_ths), len(iou_ths), 3), dtype=np.int64)
    for img in range(n_images):
        gi, pi = np.flatnonzero(g_idx == img), np.flatnonzero(p_idx == img)
        iou = np.array([[box_iou(g_xy[a], p_xy[b]) for b in pi] for a in gi], dtype=np.float64).reshape(len(gi), len(pi))
        for k, th in enumerate(conf_ths):
            g_on, p_on = g_cf[gi].astype(np.float64) > th, p_cf[pi].astype(np.float64) > th
            for t, it in enumerate(iou_ths):
                with np.errstate(invalid='ignore'):
                    pair = (iou > it) & g_on[:, None] & p_on[None, :]
                g_hit, p_hit = pair.any(axis=1).sum(), pair.any(axis=0).sum()
                out[k, t] += (g_hit, p_on.sum() - p_hit, g_on.sum() - g_hit)
    return out

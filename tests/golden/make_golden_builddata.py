#!/usr/bin/env python
"""Generate tests/golden/builddata.npz by RUNNING THE REFERENCE's box arithmetic, like make_golden_pipeline.py.

    CAPSYOLO_REFERENCE=<checkout> MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_builddata.py

Needs the reference checkout (CAPSYOLO_REFERENCE) at generation time only.  The fixture holds data only: boxes with their frame size,
input side and grid, what the reference's utils.resize_box_xy / xy_to_cwh / normalize_box_cwh returned for them, and three label
grids assembled from those functions the way build_data.py does it (its loop is restated here because build_data.py itself imports
cv2): lines 84-103 (a taken cell is skipped) for grid0 and grid1, lines 249-255 (a later box overwrites the five numbers, the earlier
class bit stays) for grid2.  grid1 and grid2 hold a cell conflict.
"""
import os
import sys

os.environ.setdefault('MPLBACKEND', 'Agg')
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('CAPSYOLO_REFERENCE')
if not REF:
    raise SystemExit('set CAPSYOLO_REFERENCE to a checkout of the reference project')
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
import utils as ref_utils          # noqa: E402

C = 43


def one_box(hw, side, g, box):
    resized = ref_utils.resize_box_xy(hw, (side, side), box)
    cwh = ref_utils.xy_to_cwh(resized)
    norm, pos = ref_utils.normalize_box_cwh((side, side), g, cwh)
    return resized, cwh, norm, pos


def box_cases():
    rng = np.random.default_rng(2024)
    rows = []
    for hw, side, g in (((800, 1360), 448, 14), ((800, 1360), 416, 13), ((600, 900), 224, 7), ((97, 131), 64, 2), ((480, 640), 608, 19)):
        h, w = hw
        for _ in range(7):
            bw, bh = rng.integers(8, min(h, w) // 4, 2)
            x1, y1 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
            # gt.txt holds integers; the augmented labels are truncated ones too, the decoded predictions are not: both kinds
            box = [x1, y1, x1 + bw, y1 + bh] if rng.random() < 0.5 else [float(int(x1)), float(int(y1)), float(int(x1) + bw), float(int(y1) + bh)]
            rows.append((h, w, side, g, box))
    # centres exactly on a cell boundary: frame 100 x 200 at side 64, grid 4 -> cells of 16; orig centre (100, 50) -> resized (32, 32)
    rows.append((100, 200, 64, 4, [90.0, 40.0, 110.0, 60.0]))
    rows.append((100, 200, 64, 4, [140.0, 65.0, 160.0, 85.0]))           # centre (150, 75) -> (48, 48)
    rows.append((800, 1360, 448, 14, [670.0, 390.0, 690.0, 410.0]))      # centre (680, 400) -> (224, 224) = 7 cells of 32
    rows.append((800, 1360, 416, 13, [1010.0, 190.0, 1030.0, 210.0]))    # centre (1020, 200) -> (312, 104): not exact in double
    rows.append((97, 131, 64, 2, [60.5, 43.5, 70.5, 53.5]))              # centre (65.5, 48.5) = the frame's centre -> (32, 32)
    return rows


def grid(hw, side, g, boxes, overwrite):
    y = np.zeros((g, g, 5 + C))
    conflicts = 0
    for x1, y1, x2, y2, c in boxes:
        _, _, (xc, yc, w, h), (row, col) = one_box(hw, side, g, [x1, y1, x2, y2])
        if not overwrite and y[row, col, 0] == 1:
            conflicts += 1
            continue
        if overwrite and y[row, col, 0] == 1:
            conflicts += 1
        y[row, col, 0:5] = [1, xc, yc, w, h]
        y[row, col, 5 + int(c)] = 1
    return y, conflicts


if __name__ == '__main__':
    arrays = {}
    rows = box_cases()
    out = [one_box((h, w), side, g, box) for h, w, side, g, box in rows]
    arrays['box_hw'] = np.array([(h, w) for h, w, _, _, _ in rows], dtype=np.int64)
    arrays['box_side'] = np.array([r[2] for r in rows], dtype=np.int64)
    arrays['box_grid'] = np.array([r[3] for r in rows], dtype=np.int64)
    arrays['box_xy'] = np.array([r[4] for r in rows], dtype=np.float64)
    arrays['box_resized'] = np.array([o[0] for o in out], dtype=np.float64)
    arrays['box_cwh'] = np.array([o[1] for o in out], dtype=np.float64)
    arrays['box_norm'] = np.array([o[2] for o in out], dtype=np.float64)
    arrays['box_pos'] = np.array([o[3] for o in out], dtype=np.int64)
    on_boundary = sum(1 for o in out if o[2][0] == 0.0 or o[2][1] == 0.0)
    print('%d boxes, %d with a normalised centre coordinate of exactly 0' % (len(rows), on_boundary))
    assert len(rows) >= 40 and on_boundary >= 3
    grids = [((800, 1360), 448, 14, [[100, 100, 140, 150, 3], [700, 300, 760, 350, 17], [1200, 600, 1250, 660, 42]], False),
             ((800, 1360), 448, 14, [[100, 100, 140, 150, 3], [110, 105, 150, 140, 9], [900, 500, 930, 540, 1]], False),
             ((97, 131), 64, 2, [[10, 10, 30, 30, 5], [20, 12, 44, 36, 7], [80, 60, 120, 90, 5]], True)]
    for k, (hw, side, g, boxes, overwrite) in enumerate(grids):
        y, conflicts = grid(hw, side, g, boxes, overwrite)
        print('grid%d: %d object cells, %d conflicts' % (k, int(y[..., 0].sum()), conflicts))
        assert conflicts == (0, 1, 1)[k]
        arrays.update({'grid%d_hw' % k: np.array(hw, dtype=np.int64), 'grid%d_side' % k: np.int64(side), 'grid%d_g' % k: np.int64(g),
                       'grid%d_boxes' % k: np.array(boxes, dtype=np.float64), 'grid%d_overwrite' % k: np.int64(overwrite),
                       'grid%d_conflicts' % k: np.int64(conflicts), 'grid%d_y' % k: y})
    assert arrays['grid2_y'][0, 0, 5:].sum() == 2                          # the overwritten cell keeps both class bits
    path = os.path.join(HERE, 'builddata.npz')
    np.savez_compressed(path, **arrays)
    print('builddata.npz %.1f KB' % (os.path.getsize(path) / 1024.0))

#!/usr/bin/env python
"""Time the suppression step (csrc/nms.hip, `cy_nms_boxes`: both launches) at the list sizes of the detectors.

    python tools/bench_nms.py [--reps 200] [--iou 0.45]

(images, boxes per image): (1, 338) is a 13 x 13 grid with two boxes per cell with every box a candidate, (1, 722) a 19 x 19 grid,
(32, 722) a batch of 32 such images.  The boxes are clustered (24 x 24 .. 48 x 48 pixels around 80 centres per image in a 608 x 608
frame), so that a good part of them is suppressed and the greedy sweep has hundreds of kept boxes, each one barrier, to walk.  Prints
one JSON line: per case the device time of one call (device events around `reps` back-to-back calls after a warm-up) and the
survivors."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd._lib import call  # noqa: E402


def boxes(n_images, per_image, seed):
    rng = np.random.RandomState(seed)
    n = n_images * per_image
    img = np.repeat(np.arange(n_images, dtype=np.int32), per_image)
    centres = rng.uniform(40.0, 568.0, (n_images, 80, 2))
    c = centres[img, rng.randint(0, 80, n)] + rng.normal(0.0, 8.0, (n, 2))
    wh = rng.uniform(24.0, 48.0, (n, 2))
    return img, np.concatenate([c - wh / 2, c + wh / 2], axis=1), rng.uniform(0.01, 1.0, n).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--iou', type=float, default=0.45)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_nms needs a GPU')
    stream = torch.cuda.current_stream().cuda_stream
    out = {'reps': a.reps, 'iou_th': a.iou, 'cases': []}
    for n_images, per_image in ((1, 338), (1, 722), (32, 722)):
        img, xy, conf = boxes(n_images, per_image, 11)
        n = len(img)
        d_img, d_xy, d_conf = (torch.from_numpy(v).cuda() for v in (img, xy, conf))
        keep, o_img, o_src = (torch.zeros(n, dtype=torch.int32, device='cuda') for _ in range(3))
        o_xy = torch.zeros((n, 4), dtype=torch.float64, device='cuda')
        o_conf = torch.zeros(n, dtype=torch.float32, device='cuda')
        words = torch.tensor([n, 0, 0] + [0] * n_images, dtype=torch.int32).cuda()      # list length, survivors, error word, scratch
        w = words.data_ptr()

        def launch():
            call('cy_nms_boxes', w, d_img.data_ptr(), d_xy.data_ptr(), d_conf.data_ptr(), None, n, n_images, a.iou, 0, 0, per_image,
                 keep.data_ptr(), n, o_img.data_ptr(), o_xy.data_ptr(), o_conf.data_ptr(), None, o_src.data_ptr(), w + 4, w + 12, w + 8,
                 stream)

        for _ in range(10):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        wd = words.cpu().numpy()
        if wd[2] != 0 or wd[1] != int(keep.sum().item()):
            raise SystemExit('cy_nms_boxes: error word %d, %d survivors counted, %d kept' % (wd[2], wd[1], int(keep.sum().item())))
        out['cases'].append({'images': n_images, 'per_image': per_image, 'survivors': int(wd[1]),
                             'call_us': 1e3 * e0.elapsed_time(e1) / a.reps})
    print(json.dumps(out))


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Time the fused composite-and-resize kernel (csrc/augment.hip, capsyolo_amd.augment.paste_resize_device) on one training batch of
GTSDB-sized frames: 32 frames of 800 x 1360 resized to 416 x 416 as centred float32 NCHW, with no paste and with 6 pastes per frame
(3 signs resized into boxes of 32 .. 128 pixels, 3 copied 1:1), against predict_fns.PackedImages.resize on the same frames -- the
float kernel that did the paste-free part before (raw 0..255 scale, same output size and layout): the yardstick.

    python tools/bench_augment.py [--reps 100] [--warmup 20] [--out profiles/augment.json]

Same process, same packed frames.  Every repetition is one call (the host's plan upload and the read-back of the error word
included: that is what a training step waits for) bracketed by its own pair of device events; the three paths alternate repetition
by repetition; the figure is the median of the repetitions after the warm-up.  A second set of figures times the bare launches
through the C-ABI with the arguments already on the device.  Prints one JSON line (and writes it to --out) with the medians in
microseconds, the 10th / 90th percentiles and the bytes each path moves at the least: the 4 x 3 tap bytes per output pixel
it asks for (taps shared by neighbouring pixels are served by the caches) and the output it stores."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import _lib, augment  # noqa: E402
from capsyolo_amd.predict_fns import PackedImages  # noqa: E402

N, H, W, SIDE = 32, 800, 1360, 416


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)          # microseconds


def scene():
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    signs, rois = [], []
    for _ in range(64):
        h, w = (int(v) for v in rng.integers(30, 121, 2))
        signs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        rois.append([3, h - 3, 3, w - 3])
    bank = augment.SignBank(signs, rois, rng.integers(0, 43, 64))
    boxes = []
    for _ in range(N):
        rows = []
        for _ in range(3):
            bw, bh = (int(v) for v in rng.integers(32, 129, 2))
            x, y = int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh))
            rows.append([x, y, x + bw, y + bh, 0])
        boxes.append(np.array(rows, dtype=np.float64))
    return frames, bank, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment needs a GPU')
    if a.reps < 50:
        raise SystemExit('bench_augment: at least 50 repetitions')
    frames, bank, boxes = scene()
    packed = PackedImages(frames)
    idx = np.arange(N)
    rect, begin, pastes, _ = augment.plan_batch(idx, packed.hw, boxes, bank, 3, 0, 0, SIDE, 13, 43)
    assert len(pastes) == 6 * N
    none = np.zeros(N + 1, np.int32)
    out = torch.empty((N, 3, SIDE, SIDE), dtype=torch.float32, device='cuda')
    paths = {'paste0': lambda: augment.paste_resize_device(packed, None, idx, rect, none, None, SIDE, SIDE, 'f32_nchw', into=out),
             'paste6': lambda: augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, SIDE, SIDE, 'f32_nchw', into=out),
             'resize_f32': lambda: packed.resize(SIDE, to_nchw=True)}
    # the bare launches: arguments uploaded once, no read-back
    sg = bank.packed('cuda')
    words = torch.from_numpy(np.concatenate([idx, rect.reshape(-1), begin, none, pastes.reshape(-1), [0]]).astype(np.int32)).cuda()
    p = words.data_ptr()
    p_rect, p_begin, p_none, p_rows, p_err = p + 4 * N, p + 20 * N, p + 4 * (6 * N + 1), p + 4 * (7 * N + 2), p + 4 * (len(words) - 1)
    stream = torch.cuda.current_stream().cuda_stream
    frame_args = (packed.buf.data_ptr(), packed.off.data_ptr(), packed.hw32.data_ptr(), packed.n, packed.nbytes)
    sign_args = (sg.buf.data_ptr(), sg.off.data_ptr(), sg.hw32.data_ptr(), sg.n, sg.nbytes)
    rect_for_crop = words[N:5 * N]
    out_crop = torch.empty((N, 3, SIDE, SIDE), dtype=torch.float32, device='cuda')
    paths.update({
        'paste0_launch': lambda: _lib.call('cy_paste_resize_u8', *frame_args, *sign_args, p, p_rect, p_none, N, p_rows, len(pastes),
                                           SIDE, SIDE, 2, out.data_ptr(), p_err, stream),
        'paste6_launch': lambda: _lib.call('cy_paste_resize_u8', *frame_args, *sign_args, p, p_rect, p_begin, N, p_rows, len(pastes),
                                           SIDE, SIDE, 2, out.data_ptr(), p_err, stream),
        'resize_f32_launch': lambda: _lib.call('cy_crop_resize_u8', *frame_args, p, rect_for_crop.data_ptr(), N, SIDE, SIDE, 0.0, 1.0, 1,
                                               out_crop.data_ptr(), p_err, stream)})
    times = {k: [] for k in paths}
    for r in range(a.warmup + a.reps):
        for k, fn in paths.items():
            us = timed(fn)
            if r >= a.warmup:
                times[k].append(us)
    torch.cuda.synchronize()
    assert int(words[-1].item()) == 0
    # the integer rule rounds what the float kernel interpolates: the two paste-free outputs agree to half a grey level
    diff = float(((paths['paste0']() * 128 + 128) - paths['resize_f32']()).abs().max().item())
    px = N * SIDE * SIDE
    result = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'frames': [N, H, W], 'side': SIDE,
              'pastes_per_frame': 6, 'max_abs_diff_grey_levels': diff,
              'bytes': {'frames_resident': packed.nbytes, 'signs_resident': sg.nbytes, 'tap_bytes_requested': px * 4 * 3,
                        'output_f32': px * 3 * 4, 'plan_upload_paste6': int(4 * (6 * N + 2 + 9 * len(pastes)))}}
    for k, v in times.items():
        result[k + '_us'] = float(np.median(v))
        result[k + '_p10_p90_us'] = [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

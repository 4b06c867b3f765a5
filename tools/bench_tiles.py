#!/usr/bin/env python
"""Latency of one camera frame through serve.SignDetector without tiles and with a 2 x 3 tiling, and the tiled decode kernel alone.

    python tools/bench_tiles.py [--reps 100] [--warmup 10] [--height 800] [--width 1360] [--rows 2 --cols 3 --overlap 128] [--graph]
                                [--plain_only]

Default-initialised DarkNet (416 x 416 input, 13 x 13 grid, 2 boxes, no classes) and CapsuleNet (43 classes, 32 x 32 crops), one
synthetic frame of the GTSDB size, suppression at IoU 0.45, a confidence threshold between two of the untiled detector's own
confidences.  Prints one JSON line:
  plain / tiled   wall milliseconds per `detect` call (host clock around the call, which ends in the wait for the record): the two
                  detectors ALTERNATE twice, `reps` calls after `warmup` each time, so that the spread between two measurements of the
                  same code stands next to the difference; `median_ms` holds the two medians, `p50_p90_p99` the percentiles over all
                  calls of a kind, `boxes` the survivors.  --graph: both detectors replay a captured graph.
  forward_ms      the detector's eval forward alone on the batch of T tiles (device events around `reps` calls): the floor of `tiled`
  decode_us       `cy_yolo_decode_tiles_conf` alone on that batch's output shape, and `cy_yolo_decode_boxes_conf` on the same batch
                  beside it (device events around `reps` back-to-back calls)
--plain_only measures `plain` alone (it is also what a tree without capsyolo_amd.tiles gets), the figure to compare between two
commits: without `tiles` the detector issues the launches it issued before the argument existed."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import models, predict_fns, serve, synth  # noqa: E402
from capsyolo_amd._lib import call  # noqa: E402

try:
    from capsyolo_amd.tiles import TileSpec  # noqa: E402
except ImportError:
    TileSpec = None


def _all_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _device_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1360)
    ap.add_argument('--rows', type=int, default=2)
    ap.add_argument('--cols', type=int, default=3)
    ap.add_argument('--overlap', type=int, default=128)
    ap.add_argument('--max_boxes', type=int, default=16)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--plain_only', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_tiles needs a GPU')
    if a.reps < 50:
        raise SystemExit('--reps %d: a median over fewer than 50 calls is not reported' % a.reps)
    plain_only = a.plain_only or TileSpec is None
    K, g, nb, side = a.max_boxes, 13, 2, 416
    dp = types.SimpleNamespace(model='darknet_d', n_classes=0, n_grid=g, n_boxes=nb, darknet_input=side, capsule_input=32, dropout=0.0,
                               device='cuda')
    cp = types.SimpleNamespace(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(0)
    dark, caps = models.DarkNet(dp).cuda().eval(), models.CapsuleNet(cp).cuda().eval()
    big = max(a.height, a.width)
    frame = np.ascontiguousarray(synth.raw_images(1, seed=7, min_side=big, max_side=big)[0][:a.height, :a.width])
    with torch.no_grad():
        y = dark(predict_fns.PackedImages([frame]).resize(side, to_nchw=True)).data
    conf = np.unique(y[..., 0::5].cpu().numpy())[::-1].astype(np.float64)
    k = min(K // 2, len(conf) - 1)
    conf_th = float(conf[k - 1] + conf[k]) / 2 if k >= 1 else float(conf[0]) - 1e-3

    kw = dict(max_boxes=K, conf_th=conf_th, graph=a.graph, nms_iou=0.45)
    dets = {'plain': serve.SignDetector(dark, dp, caps, cp, **kw)}
    if not plain_only:
        spec = TileSpec(a.rows, a.cols, a.overlap)
        dets['tiled'] = serve.SignDetector(dark, dp, caps, cp, tiles=spec, **kw)
    out = {'frame': [a.height, a.width], 'max_boxes': K, 'reps': a.reps, 'graph': a.graph, 'conf_th': conf_th}
    boxes, med, calls = {}, {}, {}
    for name, det in dets.items():
        res = det.detect(frame)
        if res.bad['boxes'] or res.bad['frames']:
            raise SystemExit('%s: %s' % (name, res.bad))
        boxes[name], med[name], calls[name] = res.total, [], []
    for _ in range(2):
        for name, det in dets.items():
            ms = _all_ms(lambda: det.detect(frame), a.reps, a.warmup)
            med[name].append(float(np.median(ms)))
            calls[name].extend(ms)
    for name in dets:
        out[name] = {'median_ms': med[name], 'p50_p90_p99': [float(v) for v in np.percentile(calls[name], [50, 90, 99])],
                     'boxes': boxes[name]}
    if not plain_only:
        T = spec.n_tiles
        out['tiles'] = {'rows': a.rows, 'cols': a.cols, 'overlap': a.overlap, 'n': T}
        rects = spec.rects(a.height, a.width)
        packed = predict_fns.PackedImages([frame])
        x = packed.crop_resize(np.zeros(T, np.int32), rects, side, side, 0.0, 1.0, True)
        with torch.no_grad():
            out['forward_ms'] = _device_ms(lambda: dark(x), a.reps, a.warmup)
            yt = dark(x).data.to(dtype=torch.float32).contiguous()
        cap = T * g * g * nb
        stream = torch.cuda.current_stream().cuda_stream
        tf = torch.zeros(T, dtype=torch.int32, device='cuda')
        tr = torch.from_numpy(np.ascontiguousarray(rects)).cuda()
        hw32 = torch.tensor([[a.height, a.width]], dtype=torch.int32).cuda()
        hw64 = torch.from_numpy(np.stack([rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2]], axis=1).astype(np.int64)).cuda()
        words = torch.zeros(3, dtype=torch.int32, device='cuda')
        idx = torch.zeros(cap, dtype=torch.int32, device='cuda')
        xy = torch.zeros((cap, 4), dtype=torch.float64, device='cuda')
        cf = torch.zeros(cap, dtype=torch.float32, device='cuda')
        w = words.data_ptr()

        def tiles_decode():
            call('cy_yolo_decode_tiles_conf', yt.data_ptr(), tf.data_ptr(), tr.data_ptr(), hw32.data_ptr(), 1, spec.margin, T, g, nb, 0,
                 0.0, w, w + 4, idx.data_ptr(), xy.data_ptr(), None, cf.data_ptr(), None, cap, w + 8, stream)

        def plain_decode():
            call('cy_yolo_decode_boxes_conf', yt.data_ptr(), hw64.data_ptr(), float(side), float(side), T, g, nb, 0, 0.0, w,
                 idx.data_ptr(), xy.data_ptr(), None, cf.data_ptr(), cap, stream)

        out['decode_us'] = {'cells': cap, 'tiles_conf': 1e3 * _device_ms(tiles_decode, a.reps, a.warmup),
                            'boxes_conf': 1e3 * _device_ms(plain_decode, a.reps, a.warmup)}
        tiles_decode()
        out['decode_us']['kept'] = int(words[0].item())
    print(json.dumps(out))


if __name__ == '__main__':
    main()

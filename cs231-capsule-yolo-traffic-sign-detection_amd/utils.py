"""Training- and prediction-side utilities with the reference's names (utils.py:14-60, 122-148, 288-351)."""
import json
import os
import shutil

import numpy as np
import torch


class Params():
    """utils.py:14-31."""

    def __init__(self, json_path):
        self.update(json_path)

    def save(self, json_path):
        with open(json_path, 'w') as f:
            json.dump({k: v for k, v in self.__dict__.items() if isinstance(v, (int, float, str, bool, list))}, f,
                      indent=4)

    def update(self, json_path):
        with open(json_path) as f:
            self.__dict__.update(json.load(f))

    @property
    def dict(self):
        return self.__dict__


def save_checkpoint(state, is_best, checkpoint):
    """utils.py:40-49: <dir>/last.pth.tar (+ best.pth.tar copy)."""
    filepath = os.path.join(checkpoint, 'last.pth.tar')
    if not os.path.exists(checkpoint):
        os.makedirs(checkpoint)
    torch.save(state, filepath)
    if is_best:
        shutil.copyfile(filepath, os.path.join(checkpoint, 'best.pth.tar'))


class NoEmaInCheckpoint(ValueError):
    """--use_ema on a checkpoint that was written without --ema."""


def load_checkpoint(checkpoint, model, params=None, optimizer=None):
    """utils.py:52-60 (the reference raises a str on a missing file; a real exception here).
    An 'ema_state_dict' entry (main.py --ema: the optimizer's moving averages under the model's parameter names) goes back into an
    optimizer that keeps averages; a checkpoint without the entry loads as it always did.  params.use_ema (main.py --use_ema, the
    modes that only run the model): the averaged values become the model's parameters; True needs the entry (NoEmaInCheckpoint
    otherwise), 'if_present' takes it when it is there.  Buffers are the checkpoint's 'state_dict' ones either way."""
    if not os.path.exists(checkpoint):
        raise FileNotFoundError("File doesn't exist {}".format(checkpoint))
    ckpt = torch.load(checkpoint, map_location='cpu', weights_only=False)
    model.load_state_dict(ckpt['state_dict'])
    if optimizer and 'optim_dict' in ckpt:
        optimizer.load_state_dict(ckpt['optim_dict'])
    if optimizer and getattr(optimizer, 'ema_decay', None) is not None and 'ema_state_dict' in ckpt:
        optimizer.load_ema_state_dict(model, ckpt['ema_state_dict'])
    use_ema = getattr(params, 'use_ema', False) if params is not None else False
    if use_ema:
        if 'ema_state_dict' in ckpt:
            from . import ops
            ema = ckpt['ema_state_dict']
            bad = [name for name, p in model.named_parameters() if name not in ema or tuple(ema[name].shape) != tuple(p.shape)]
            if bad:
                raise ValueError("--use_ema: the 'ema_state_dict' of {} does not fit this model: no entry of the parameter's shape for {}"
                                 .format(checkpoint, ', '.join(bad[:5]) + (' ...' if len(bad) > 5 else '')))
            with torch.no_grad():
                for name, p in model.named_parameters():
                    p.copy_(ema[name])
            ops._bump_param_epoch()
            print("Using the averaged (EMA) parameters of {}".format(checkpoint))
        elif use_ema != 'if_present':
            raise NoEmaInCheckpoint("--use_ema: {} has no 'ema_state_dict' entry: it was written by a training run without --ema"
                                    .format(checkpoint))
    return ckpt


def load_data(data_dir, is_small=False, npy=False):
    """utils.py:91-113: pickle (X, Y) tuples or *_X.npy / *_Y.npy pairs."""
    import pickle
    from . import config
    tr = data_dir + (config.tr_sm_d if is_small else config.tr_d)
    ev = data_dir + (config.ev_sm_d if is_small else config.ev_d)
    if not npy:
        with open(tr, 'rb') as f:
            x_tr, y_tr = pickle.load(f)
        with open(ev, 'rb') as f:
            x_ev, y_ev = pickle.load(f)
        return x_tr, y_tr, x_ev, y_ev
    tr, ev = tr.split('.')[0], ev.split('.')[0]
    return np.load(tr + '_X.npy'), np.load(tr + '_Y.npy'), np.load(ev + '_X.npy'), np.load(ev + '_Y.npy')


def center_rgb(x):
    """utils.py:122-123."""
    return (x - 128) / 128


def shuffle(x, y):
    """utils.py:146-148."""
    i = np.random.permutation(len(y))
    return x[i], y[i]


def decode_boxes_device(y, params, image_hw=None, conf_th=0.5, with_conf=False):
    """`cy_yolo_decode_boxes` with everything left on the device: (n, image_idx int32[n], xy float64[n,4], cls int32[n] | None);
    with_conf: `cy_yolo_decode_boxes_conf`, which appends the stored confidence of every box (float32[n])."""
    from ._lib import call
    yt = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(device='cuda', dtype=torch.float32).contiguous()
    batch, g, _, D = yt.shape
    C = int(params.n_classes)
    nb = int((D - C) / 5)
    if nb < 1:          # e.g. DarkCapsuleNet's [B,g,g,5] output with n_classes = 43: the reference's reshape fails here too
        raise ValueError('y has %d values per cell: no box left after %d class scores (utils.py:291-293)' % (D, C))
    cap = batch * g * g * nb
    dev = yt.device
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    idx = torch.empty(cap, dtype=torch.int32, device=dev)
    xy = torch.empty((cap, 4), dtype=torch.float64, device=dev)
    cls = torch.empty(cap, dtype=torch.int32, device=dev) if C else None
    hw = None
    if image_hw is not None:
        hw = torch.as_tensor(np.ascontiguousarray(np.asarray(image_hw).reshape(batch, 2)), dtype=torch.int64).to(dev)
    side = float(params.darknet_input)
    stream = torch.cuda.current_stream().cuda_stream
    if with_conf:
        conf = torch.empty(cap, dtype=torch.float32, device=dev)
        call('cy_yolo_decode_boxes_conf', yt.data_ptr(), hw.data_ptr() if hw is not None else None, side, side, batch, g, nb, C,
             float(conf_th), count.data_ptr(), idx.data_ptr(), xy.data_ptr(), cls.data_ptr() if C else None, conf.data_ptr(), cap,
             stream)
        n = int(count.item())
        return n, idx[:n], xy[:n], (cls[:n] if C else None), conf[:n]
    call('cy_yolo_decode_boxes', yt.data_ptr(), hw.data_ptr() if hw is not None else None, side, side, batch, g, nb, C,
         float(conf_th), count.data_ptr(), idx.data_ptr(), xy.data_ptr(), cls.data_ptr() if C else None, cap, stream)
    n = int(count.item())
    return n, idx[:n], xy[:n], (cls[:n] if C else None)


def decode_tiles_device(y, params, tile_frame, tile_rect, frame_hw, conf_th=0.5, margin=2.0, with_tile=False, max_boxes=None):
    """`cy_yolo_decode_tiles_conf` with everything left on the device: y [Bt, g, g, D] is the detector's output for Bt tiles, tile b
    being rectangle tile_rect[b] = (y0, y1, x0, x1) of frame tile_frame[b] (ascending), frame_hw [n, 2] = (height, width) of the
    frames.  Returns (n, idx int32[n], xy float64[n,4] in frame pixels, cls int32[n] | None, conf float32[n], dropped[, tile int32[n]]):
    the boxes the border rule kept (include/capsyolo_hip.h; margin < 0: all) in (tile, row, column, box) order, idx = their frames,
    dropped = how many the rule dropped, tile = the tile each came from.  max_boxes: output slots (default: all Bt g^2 nb); n may
    exceed it, min(n, max_boxes) entries are returned.  A bad tile raises ValueError."""
    from ._lib import call
    yt = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(device='cuda', dtype=torch.float32).contiguous()
    Bt, g, _, D = yt.shape
    C = int(params.n_classes)
    nb = int((D - C) / 5)
    if nb < 1:
        raise ValueError('y has %d values per cell: no box left after %d class scores (utils.py:291-293)' % (D, C))
    dev = yt.device

    def table(a, shape):
        return torch.as_tensor(a if torch.is_tensor(a) else np.asarray(a)).to(device=dev, dtype=torch.int32).reshape(shape).contiguous()
    tf, tr, hw = table(tile_frame, (-1,)), table(tile_rect, (-1, 4)), table(frame_hw, (-1, 2))
    if int(tf.numel()) != Bt or int(tr.shape[0]) != Bt or int(hw.shape[0]) < 1:
        raise ValueError('decode_tiles_device: y has %d tiles, tile_frame %d, tile_rect %d, frame_hw %d frames'
                         % (Bt, tf.numel(), tr.shape[0], hw.shape[0]))
    cap = Bt * g * g * nb if max_boxes is None else int(max_boxes)
    words = torch.zeros(3, dtype=torch.int32, device=dev)                 # count, dropped, error word
    idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    xy = torch.empty((max(cap, 1), 4), dtype=torch.float64, device=dev)
    cls = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if C else None
    conf = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
    tile = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if with_tile else None
    w = words.data_ptr()
    call('cy_yolo_decode_tiles_conf', yt.data_ptr(), tf.data_ptr(), tr.data_ptr(), hw.data_ptr(), int(hw.shape[0]), float(margin), Bt, g, nb,
         C, float(conf_th), w, w + 4, idx.data_ptr(), xy.data_ptr(), cls.data_ptr() if C else None, conf.data_ptr(),
         tile.data_ptr() if with_tile else None, cap, w + 8, torch.cuda.current_stream().cuda_stream)
    n, dropped, err = (int(v) for v in words.cpu().numpy())
    if err:
        raise ValueError('decode_tiles_device: %d tile(s) with a frame index outside 0..%d or a rectangle that is empty or leaves its frame'
                         % (err, hw.shape[0] - 1))
    m = min(n, cap)
    out = (n, idx[:m], xy[:m], (cls[:m] if C else None), conf[:m], dropped)
    return out + (tile[:m],) if with_tile else out


def _nms_call(count, idx, xy, conf, cls, n_cap, n_images, iou_th, class_aware, per_image, max_per_image, K):
    """`cy_nms_boxes` on a device list (count: int32 [1] device tensor): (keep int32 [n_cap], out_img, out_xy, out_conf, out_cls | None,
    out_src, words int32 [2] = (survivors, error word)), all on the device, nothing read back."""
    from ._lib import call
    dev = idx.device
    keep = torch.zeros(max(n_cap, 1), dtype=torch.int32, device=dev)
    out_img = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
    out_xy = torch.zeros((max(K, 1), 4), dtype=torch.float64, device=dev)
    out_conf = torch.zeros(max(K, 1), dtype=torch.float32, device=dev)
    out_cls = torch.zeros(max(K, 1), dtype=torch.int32, device=dev) if cls is not None else None
    out_src = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
    words = torch.zeros(2 + n_images, dtype=torch.int32, device=dev)       # survivors, error word, per-image scratch
    call('cy_nms_boxes', count.data_ptr(), idx.data_ptr(), xy.data_ptr(), conf.data_ptr(), cls.data_ptr() if cls is not None else None,
         int(n_cap), int(n_images), float(iou_th), int(bool(class_aware)), int(per_image), int(max_per_image), keep.data_ptr(), int(K),
         out_img.data_ptr(), out_xy.data_ptr(), out_conf.data_ptr(), out_cls.data_ptr() if cls is not None else None,
         out_src.data_ptr(), words.data_ptr(), words.data_ptr() + 8, words.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    return keep[:n_cap], out_img[:K], out_xy[:K], out_conf[:K], (out_cls[:K] if cls is not None else None), out_src[:K], words[:2]


def _check_nms_args(iou_th, per_image):
    if not (0.0 <= float(iou_th) <= 1.0):
        raise ValueError('iou_th must be in [0, 1], got %r' % (iou_th,))
    if int(per_image) != per_image or per_image < 0:
        raise ValueError('per_image must be an integer >= 0, got %r' % (per_image,))


def nms_boxes_device(image_indices, boxes_xy, conf, classes=None, iou_th=0.45, class_aware=False, per_image=0, n_images=None,
                     max_out=None):
    """Greedy confidence-ordered non-maximum suppression of a decoded box list on the device (`cy_nms_boxes`; the rule is in
    include/capsyolo_hip.h).  image_indices [n] ascending, boxes_xy [n, 4] = (x1, y1, x2, y2), conf [n], classes [n] or None: arrays
    or tensors, e.g. what decode_boxes_device(..., with_conf=True) returned.  n_images: default max(image_indices) + 1; max_out:
    output slots, default n.  Returns (n_kept, idx int32, xy float64, conf float32, cls int32 | None, src int32, keep int32 [n]) as
    device tensors: the survivors, image ascending and inside an image confidence descending (src: their positions in the input;
    min(n_kept, max_out) of them are returned), and the keep mask in input order.  The one-shot form: it reads the count back."""
    from ._lib import query
    _check_nms_args(iou_th, per_image)
    if class_aware and classes is None:
        raise ValueError('class_aware suppression needs the classes')

    def dev_t(a, dtype):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device='cuda', dtype=dtype).contiguous()
    idx = dev_t(image_indices, torch.int32).reshape(-1)
    xy = dev_t(boxes_xy, torch.float64).reshape(-1, 4)
    cf = dev_t(conf, torch.float32).reshape(-1)
    cls = dev_t(classes, torch.int32).reshape(-1) if classes is not None else None
    n = int(idx.numel())
    if int(xy.shape[0]) != n or int(cf.numel()) != n or (cls is not None and int(cls.numel()) != n):
        raise ValueError('nms_boxes_device: %d image indices, %d boxes, %d confidences%s'
                         % (n, xy.shape[0], cf.numel(), '' if cls is None else ', %d classes' % cls.numel()))
    K = n if max_out is None else int(max_out)
    if max_out is not None and K < 1:   # (the entry point launches nothing for no slots, so there would be no mask either)
        raise ValueError('max_out must be >= 1, got %r' % (max_out,))
    if n_images is None:
        n_images = int(idx.max().item()) + 1 if n else 1
    if n == 0:
        empty = torch.zeros(0, dtype=torch.int32, device=idx.device)
        return (0, empty, torch.zeros((0, 4), dtype=torch.float64, device=idx.device), torch.zeros(0, dtype=torch.float32, device=idx.device),
                (empty.clone() if cls is not None else None), empty.clone(), torch.zeros(n, dtype=torch.int32, device=idx.device))
    count = torch.full((1,), n, dtype=torch.int32, device=idx.device)
    cap = min(n, int(query('cy_nms_max_per_image')))
    keep, o_img, o_xy, o_conf, o_cls, o_src, words = _nms_call(count, idx, xy, cf, cls, n, n_images, iou_th, class_aware, per_image, cap, K)
    n_kept, err = (int(v) for v in words.cpu().numpy())
    if err:
        raise ValueError('nms_boxes_device: %d image(s) have more than %d boxes, the most one block holds' % (err >> 20, cap))
    m = min(n_kept, K)
    return n_kept, o_img[:m], o_xy[:m], o_conf[:m], (o_cls[:m] if cls is not None else None), o_src[:m], keep


def nms_y_hat_device(y_hat, params, iou_th=0.45, class_aware=False, per_image=0, image_hw=None):
    """A float32 device copy of the detector output y_hat [B, g, g, 5 nb + C] in which the confidence of every box that non-maximum
    suppression removes is 0.0; every other value keeps its bits.  The candidates are all boxes with a confidence > 0, decoded with
    image_hw like decode_boxes_device does it, suppressed per image by `cy_nms_boxes`.  Greedy suppression in descending confidence
    is prefix-consistent -- whether a box survives depends on the boxes of at least its confidence alone -- so decoding the result
    at ANY threshold t >= 0 gives exactly the boxes that suppression of the boxes over t keeps: one masked y_hat serves the decode
    at 0.5 behind the crops and the drawing and every threshold of the metric sweeps.  class_aware uses the detector's own arg-max
    class and needs params.n_classes > 0."""
    _check_nms_args(iou_th, per_image)
    C = int(params.n_classes)
    if class_aware and C == 0:
        raise ValueError('class_aware suppression needs a detector with class scores (params.n_classes > 0)')
    yt = torch.as_tensor(np.asarray(y_hat) if not torch.is_tensor(y_hat) else y_hat).to(device='cuda', dtype=torch.float32).contiguous()
    out = yt.clone()
    batch, g, _, D = yt.shape
    n, idx, xy, cls, conf = decode_boxes_device(yt, params, image_hw, 0.0, with_conf=True)
    if n == 0:
        return out
    nb = int((D - C) / 5)
    confs = out[..., 0:5 * nb:5]                      # a view [B, g, g, nb] of the copy
    # the decode kernel walks (image, row, column, box) in this order and takes a box iff its float32 confidence > 0.0f: the
    # same comparison in the same order, so entry k of the list is row k of `where`
    where = torch.nonzero(confs > 0.0)
    if int(where.shape[0]) != n:
        raise AssertionError('nms_y_hat_device: the decode kernel found %d boxes, the comparison %d' % (n, where.shape[0]))
    count = torch.full((1,), n, dtype=torch.int32, device=yt.device)
    keep, _, _, _, _, _, words = _nms_call(count, idx.contiguous(), xy.contiguous(), conf.contiguous(),
                                           cls.contiguous() if class_aware else None, n, batch, iou_th, class_aware, per_image,
                                           g * g * nb, 1)
    dead = where[keep == 0]
    confs[dead[:, 0], dead[:, 1], dead[:, 2], dead[:, 3]] = 0.0
    return out


def y_to_boxes_vec(y, params, image_hw=None, conf_th=0.5):
    """utils.py:288-334 on the device (`cy_yolo_decode_boxes`): y is the network output / ground truth as a numpy
    array or a tensor, image_hw an optional (batch, 2) array of (height, width).  Returns (image_indices, xy, classes)
    as numpy arrays like the reference (classes is None when params.n_classes == 0)."""
    n, idx, xy, cls = decode_boxes_device(y, params, image_hw, conf_th)
    return (idx.cpu().numpy().astype(np.int64), xy.cpu().numpy(),
            cls.cpu().numpy().astype(np.int64) if cls is not None else None)


def crop_rectangles(boxes_xy, image_indices, image_hw):
    """The crop of every decoded box as plot.py:22 takes it, `image[int(y1):int(y2), int(x1):int(x2)]`: int64 [n, 4] =
    (y0, y1, x0, x1), half-open.  In double like the reference: the corners are truncated towards zero, then clipped to
    [0, w] x [0, h] -- which is what a slice does with a corner beyond the image.  Deliberately NOT kept: Python's wrap-around of
    a negative index (a box that leaves the image on the left would crop from the right border).  An empty rectangle raises
    ValueError naming the box (the reference dies in cv2.resize there)."""
    xy = np.asarray(boxes_xy, dtype=np.float64).reshape(-1, 4)
    idx = np.asarray(image_indices, dtype=np.int64).reshape(-1)
    hw = np.asarray(image_hw, dtype=np.int64).reshape(-1, 2)
    if len(idx) != len(xy) or (len(idx) and (idx.min() < 0 or idx.max() >= len(hw))):
        raise ValueError('crop_rectangles: %d boxes, %d image indices, %d images' % (len(xy), len(idx), len(hw)))
    if not np.all(np.isfinite(xy)):
        raise ValueError('crop_rectangles: box %d has a corner that is not finite' % int(np.argwhere(~np.isfinite(xy))[0, 0]))
    t = np.trunc(xy)
    h, w = hw[idx, 0].astype(np.float64), hw[idx, 1].astype(np.float64)
    x0, x1 = np.clip(t[:, 0], 0, w), np.clip(t[:, 2], 0, w)
    y0, y1 = np.clip(t[:, 1], 0, h), np.clip(t[:, 3], 0, h)
    rect = np.stack([y0, y1, x0, x1], axis=1).astype(np.int64)
    empty = np.argwhere((rect[:, 1] <= rect[:, 0]) | (rect[:, 3] <= rect[:, 2])).reshape(-1)
    if len(empty):
        i = int(empty[0])
        raise ValueError('box %d of image %d (x1, y1, x2, y2 = %s) is empty after clipping to %d x %d'
                         % (i, idx[i], xy[i].tolist(), hw[idx[i], 1], hw[idx[i], 0]))
    return rect


def combine_y_hat_device(image_hw, dark_y_hat, class_y_hat, image_indices, boxes_xy, params):
    """`cy_combine_scores` with everything left on the device: float32 tensor [B, g, g, D + C]."""
    from ._lib import call
    dev = torch.device('cuda')

    def dev_t(a, dtype):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=dtype).contiguous()
    dark = dev_t(dark_y_hat, torch.float32)
    scores = dev_t(class_y_hat, torch.float32)
    B, g, _, D = dark.shape
    if scores.dim() != 2 or int(scores.shape[1]) < 1:
        raise ValueError('class_y_hat must be [n_boxes, n_classes], got %s' % (tuple(scores.shape),))
    n, C = int(scores.shape[0]), int(scores.shape[1])
    if g != int(params.n_grid):
        raise ValueError('dark_y_hat has a %d x %d grid, params.n_grid is %d' % (g, g, params.n_grid))
    idx = dev_t(image_indices, torch.int32).reshape(-1)
    xy = dev_t(boxes_xy, torch.float64).reshape(-1, 4)
    hw = dev_t(np.asarray(image_hw).reshape(-1, 2), torch.int64)
    if int(idx.numel()) != n or int(xy.shape[0]) != n or int(hw.shape[0]) != B:
        raise ValueError('combine_y_hat: %d score rows, %d image indices, %d boxes; %d images for a batch of %d'
                         % (n, idx.numel(), xy.shape[0], hw.shape[0], B))
    scratch = torch.zeros(B * g * g + 1, dtype=torch.int32, device=dev)           # winning box per cell, then the error word
    y_hat = torch.empty((B, g, g, D + C), dtype=torch.float32, device=dev)
    call('cy_combine_scores', dark.data_ptr(), scores.data_ptr() if n else None, idx.data_ptr() if n else None,
         xy.data_ptr() if n else None, n, hw.data_ptr(), float(params.darknet_input), B, g, D, C, scratch.data_ptr(),
         y_hat.data_ptr(), scratch.data_ptr() + 4 * B * g * g, torch.cuda.current_stream().cuda_stream)
    bad = int(scratch[-1].item())
    if bad:
        raise ValueError('combine_y_hat: the centre of %d box(es) lies outside the %d x %d grid (or its image index outside the '
                         'batch)' % (bad, g, g))
    return y_hat


def combine_y_hat(images, dark_y_hat, class_y_hat, image_indices, boxes_xy, params):
    """utils.py:336-351 on the device (`cy_combine_scores`): the detector's output with the class scores of every box written
    behind the cell that holds the box's centre -> float64 numpy [B, g, g, D + C] like the reference.  `images` is the list of
    raw images (only their shapes are read) or an array of (height, width) rows.  Of several boxes in one cell the one with
    the highest index wins, as in the reference's loop; a centre outside the grid raises ValueError (the reference raises
    IndexError or wraps around)."""
    if isinstance(images, np.ndarray) and images.ndim == 2 and images.shape[1] == 2:
        image_hw = images
    else:
        image_hw = np.array([np.asarray(im).shape[0:2] for im in images])
    return combine_y_hat_device(image_hw, dark_y_hat, class_y_hat, image_indices, boxes_xy, params).cpu().numpy().astype(np.float64)

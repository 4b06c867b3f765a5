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


def load_checkpoint(checkpoint, model, params=None, optimizer=None):
    """utils.py:52-60 (the reference raises a str on a missing file; a real exception here)."""
    if not os.path.exists(checkpoint):
        raise FileNotFoundError("File doesn't exist {}".format(checkpoint))
    ckpt = torch.load(checkpoint, map_location='cpu', weights_only=False)
    model.load_state_dict(ckpt['state_dict'])
    if optimizer and 'optim_dict' in ckpt:
        optimizer.load_state_dict(ckpt['optim_dict'])
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

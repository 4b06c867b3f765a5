"""Prediction with the reference's names (predict_fns.py:10-82): the eval forwards, and the two-stage chain detector ->
box crops -> classifier -> combined y_hat with every step between the two forwards on the device (csrc/predict.hip).

Resizing follows cv2.resize's INTER_LINEAR half-pixel convention (source coordinate (o + 0.5) * n_in / n_out - 0.5, neighbours
clamped into the image or crop), interpolated in fp32.  cv2's 11-bit fixed-point rounding of the weights is NOT reproduced (cv2
is not a dependency, so the difference could not be measured; it is expected to stay within one grey level).  The images with the
boxes drawn (plot.draw_boxes_vec) are returned where `draw=True` asks for them, drawn on the device while a chunk's packed images
are there (draw.py, `cy_draw_boxes_u8`); the default returns None in their place and draws nothing.  JPEGs are not written."""
import os

import numpy as np
import torch

from . import draw as box_draw
from . import utils
from ._lib import call


def _restore(model, model_dir, params, restore_file):
    path = os.path.join(model_dir, restore_file + '.pth.tar')
    print("Restoring parameters from {}".format(path))
    utils.load_checkpoint(path, model, params)


def _eval_chunks(x, model, params, batch_size):
    """The reference pushes the WHOLE set through the model in one call (predict_fns.py:40-43, 65-69: x [N,3,448,448]).
    In eval mode every sample is independent (BatchNorm uses the running statistics, folded into the conv weights here:
    ops.fold_eval_bn), so the set goes through in chunks of `batch_size` with identical results and bounded memory.
    Yields each chunk's output as a device tensor."""
    n = int(x.shape[0])
    bs = n if not batch_size else int(batch_size)
    model.eval()
    with torch.no_grad():
        for lo in range(0, n, max(bs, 1)):
            xt = torch.from_numpy(np.ascontiguousarray(x[lo:lo + bs])).to(device=params.device, dtype=torch.float32)
            yield model(xt.permute(0, 3, 1, 2).contiguous()).data


def _eval_forward_batched(x, model, params, batch_size):
    outs = [o.cpu().numpy() for o in _eval_chunks(x, model, params, batch_size)]
    return np.concatenate(outs, axis=0) if len(outs) != 1 else outs[0]


def class_scores_device(x, model, params, batch_size=1024):
    """The forward of class_pred (same chunks, same kernels, so the same bits) with the scores left on the device: x NHWC numpy
    -> float32 device tensor [N, n_classes], no per-chunk copy to the host.  What metrics.recog_counts reads in place.  The
    checkpoint is the caller's business (class_pred restores it, this does not)."""
    outs = list(_eval_chunks(x, model, params, batch_size))
    if not outs:
        raise ValueError('class_scores_device: no samples')
    return torch.cat(outs, 0) if len(outs) != 1 else outs[0]


def class_pred(x, model, model_dir, params, restore_file, batch_size=1024):
    """predict_fns.py:60-73: x NHWC numpy -> (scores, argmax classes).  batch_size (new, optional): chunk of the set per forward
    call; None = the whole set at once like the reference."""
    _restore(model, model_dir, params, restore_file)
    y_hat = _eval_forward_batched(x, model, params, batch_size)
    return y_hat, np.argmax(y_hat, axis=1)


def dark_forward(x, model, model_dir, params, restore_file, batch_size=32):
    """predict_fns.py:38-43: eval forward of the detector on already-resized NHWC images -> y_hat numpy (batched like class_pred)."""
    _restore(model, model_dir, params, restore_file)
    return _eval_forward_batched(x, model, params, batch_size)


class PackedImages(object):
    """A list of HWC uint8 images of different sizes as ONE device buffer (what `cy_crop_resize_u8` reads)."""

    def __init__(self, images, device='cuda'):
        arrs = []
        for k, im in enumerate(images):
            a = np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError('image %d: expected a uint8 array [h, w, 3], got %s %s' % (k, a.dtype, a.shape))
            arrs.append(np.ascontiguousarray(a))
        if not arrs:
            raise ValueError('no images')
        self.n = len(arrs)
        self.hw = np.array([a.shape[0:2] for a in arrs], dtype=np.int64)
        sizes = np.array([a.size for a in arrs], dtype=np.int64)
        self.nbytes = int(sizes.sum())
        self.buf = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(device)
        self.off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).to(device)
        self.hw32 = torch.from_numpy(self.hw.astype(np.int32)).to(device)

    def crop_resize(self, box_img, rect, oh, ow, shift=0.0, scale=1.0, to_nchw=False):
        """float32 device tensor [n, oh, ow, 3] ([n, 3, oh, ow] with to_nchw): (resized crop + shift) * scale."""
        box_img = np.ascontiguousarray(np.asarray(box_img, dtype=np.int32).reshape(-1))
        rect = np.ascontiguousarray(np.asarray(rect, dtype=np.int32).reshape(-1, 4))
        n = len(box_img)
        if len(rect) != n:
            raise ValueError('%d image indices for %d rectangles' % (n, len(rect)))
        dev = self.buf.device
        out = torch.empty((n, 3, oh, ow) if to_nchw else (n, oh, ow, 3), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        args = torch.from_numpy(np.concatenate([rect.reshape(-1), box_img, [0]]).astype(np.int32)).to(dev)   # rect, index, error word
        call('cy_crop_resize_u8', self.buf.data_ptr(), self.off.data_ptr(), self.hw32.data_ptr(), self.n, self.nbytes,
             args.data_ptr() + 16 * n, args.data_ptr(), n, int(oh), int(ow), float(shift), float(scale), int(bool(to_nchw)),
             out.data_ptr(), args.data_ptr() + 20 * n, torch.cuda.current_stream().cuda_stream)
        bad = int(args[-1].item())
        if bad:
            raise ValueError('%d rectangle(s) are empty or reach outside their image' % bad)
        return out

    def resize(self, side, to_nchw=True):
        rect = np.stack([np.zeros(self.n, np.int64), self.hw[:, 0], np.zeros(self.n, np.int64), self.hw[:, 1]], axis=1)
        return self.crop_resize(np.arange(self.n), rect, side, side, 0.0, 1.0, to_nchw)


def resize_images_device(images, side):
    """predict_fns.py:38, `cv2.resize(image, (side, side))` of every image of a list of HWC uint8 arrays of different sizes, on the
    device in one launch: float32 tensor [n, 3, side, side] with the raw 0..255 scale the reference feeds the detector."""
    return PackedImages(images).resize(int(side), to_nchw=True)


def _chunk_size(n, batch_size):
    return max(int(batch_size) if batch_size else n, 1)


def _detect_and_crop(images, model, params, conf_th, batch_size, crop_side, shift, scale, to_nchw, drawer=None, nms=None):
    """Chunks of `batch_size` images: upload -> resize -> eval forward -> decode with the images' own sizes -> rectangles ->
    crops, all but the rectangle rule (a few integers per box, in double on the host) on the device.
    Returns (y_hat device [B,g,g,D], crops device, image_indices int64 numpy, boxes_xy float64 numpy).  drawer (optional):
    called as drawer(lo, packed, image_indices, boxes_xy, classes) with every chunk's boxes (indices inside the chunk, classes an
    int64 numpy array or None) while its packed images are on the device.  nms (optional): (iou_th, class_aware); every chunk's
    y_hat goes through utils.nms_y_hat_device with the chunk's image sizes before the decode, so the boxes, the crops, what the
    drawer sees and the returned y_hat are those of the survivors; one line says how many boxes over conf_th that removed."""
    n = len(images)
    bs = _chunk_size(n, batch_size)
    y_hats, crops, idxs, xys = [], [], [], []
    before = 0
    model.eval()
    with torch.no_grad():
        for lo in range(0, n, bs):
            packed = PackedImages(images[lo:lo + bs], params.device)
            y_hat = model(packed.resize(int(params.darknet_input), to_nchw=True)).data
            if nms is not None:
                before += utils.decode_boxes_device(y_hat, params, packed.hw, conf_th)[0]
                y_hat = utils.nms_y_hat_device(y_hat, params, nms[0], nms[1], 0, packed.hw)
            nbox, idx, xy, cls = utils.decode_boxes_device(y_hat, params, packed.hw, conf_th)
            idx_np, xy_np = idx.cpu().numpy().astype(np.int64), xy.cpu().numpy()
            if drawer is not None:
                drawer(lo, packed, idx_np, xy_np, cls.cpu().numpy().astype(np.int64) if cls is not None else None)
            try:
                rect = utils.crop_rectangles(xy_np, idx_np, packed.hw)
            except ValueError as e:
                raise ValueError('images %d..%d: %s' % (lo, lo + packed.n - 1, e))
            crops.append(packed.crop_resize(idx_np, rect, crop_side, crop_side, shift, scale, to_nchw))
            y_hats.append(y_hat)
            idxs.append(idx_np + lo)
            xys.append(xy_np)
    if nms is not None:
        after = sum(len(i) for i in idxs)
        print('nms (iou > {}{}): {} of {} boxes over {} suppressed'.format(nms[0], ', per class' if nms[1] else '', before - after, before,
                                                                           conf_th))
    return torch.cat(y_hats, 0), torch.cat(crops, 0), np.concatenate(idxs), np.concatenate(xys, 0)


def _nms_option(nms_iou, nms_class_aware, params):
    """None, or the checked (iou_th, class_aware) that _detect_and_crop takes."""
    if nms_iou is None:
        if nms_class_aware:
            raise ValueError('nms_class_aware needs nms_iou')
        return None
    if not (0.0 <= float(nms_iou) <= 1.0):
        raise ValueError('nms_iou must be in [0, 1], got %r' % (nms_iou,))
    if nms_class_aware and int(params.n_classes) == 0:
        raise ValueError('nms_class_aware needs a detector with class scores (params.n_classes > 0)')
    return float(nms_iou), bool(nms_class_aware)


def dark_pred(images, model, model_dir, params, restore_file, is_end=True, conf_th=0.5, y=None, batch_size=32, draw=False, nms_iou=None,
              nms_class_aware=False):
    """predict_fns.py:10-58.  images: list of HWC uint8 arrays of different sizes.  is_end=True: (y_hat, None), or with draw=True
    (new, optional) (y_hat, images): the reference's second value, copies of the images with the boxes over conf_th in green,
    labelled with the detector's argmax class when params.n_classes > 0, and, when the labels y [n, g, g, 5 + C] are given, the
    ground-truth boxes in red on top (predict_fns.py:46-51; decoded like the predictions, so from float32 values).  Both sets
    are drawn in one launch per chunk, ground truth last (draw.draw_boxes_device).  Without draw, y is not read.
    is_end=False: (y_hat, crops float32 numpy [n_boxes, ci, ci, 3] on the raw 0..255 scale like the reference,
    image_indices [n_boxes], boxes_xy [n_boxes, 4] in pixels of the original images).
    nms_iou (new, optional): non-maximum suppression at this IoU (utils.nms_y_hat_device; nms_class_aware: per arg-max class of the
    detector) before decode, crops and drawing; the returned y_hat has the confidence of every suppressed box set to 0.  None: no
    suppression, the reference's behaviour."""
    nms = _nms_option(nms_iou, nms_class_aware, params)
    _restore(model, model_dir, params, restore_file)
    ci = int(params.capsule_input)
    drawn = []

    def drawer(lo, packed, idx, xy, cls):
        colors = np.tile(np.array(box_draw.GREEN, dtype=np.uint8), (len(idx), 1))
        if y is not None:
            _, t_idx, t_xy, t_cls = utils.decode_boxes_device(y[lo:lo + packed.n], params, packed.hw, conf_th)
            idx = np.concatenate([idx, t_idx.cpu().numpy().astype(np.int64)])
            xy = np.concatenate([xy.reshape(-1, 4), t_xy.cpu().numpy().reshape(-1, 4)])
            if cls is not None:
                cls = np.concatenate([cls, t_cls.cpu().numpy().astype(np.int64)])
            colors = np.concatenate([colors, np.tile(np.array(box_draw.RED, dtype=np.uint8), (len(idx) - len(colors), 1))])
        drawn.extend(box_draw.unpack_images(box_draw.draw_boxes_device(packed, idx, xy, colors, cls), packed))
    want = bool(draw) and is_end
    y_hat, crops, idx, xy = _detect_and_crop(images, model, params, conf_th, batch_size, ci, 0.0, 1.0, False, drawer if want else None, nms)
    if is_end:
        return y_hat.cpu().numpy(), (drawn if want else None)
    return y_hat.cpu().numpy(), crops.cpu().numpy(), idx, xy


def dark_pred_tiled(images, model, model_dir, params, restore_file, tiles, nms_iou, conf_th=0.5, y=None, batch_size=32, draw=False,
                    nms_class_aware=False):
    """dark_pred with the detector run on the overlapping windows of every image (tiles: a tiles.TileSpec) instead of the image.
    images: list of HWC uint8 arrays of different sizes; every image gets the tile table of its own size.  Per chunk of images: one
    crop + resize of all windows, the eval forward on that batch, utils.decode_tiles_device at confidence > 0 (border rule, frame
    pixels), utils.nms_boxes_device per image at nms_iou -- once: greedy suppression in descending confidence is prefix-consistent,
    so the part of the merged list over ANY threshold is what suppressing the boxes over that threshold keeps, and one list serves
    the drawing at conf_th and every threshold of metrics.detect_report_boxes.
    Returns ((image_indices int64 [n], boxes_xy float64 [n, 4] in image pixels, conf float32 [n], classes int64 [n] | None), images):
    the merged list as numpy arrays, image ascending and inside an image confidence descending, and with draw=True copies of the
    images with the list's boxes over conf_th in green and, when the labels y are given, the ground truth in red (as dark_pred draws
    them), else None."""
    from ._lib import query
    nms = _nms_option(nms_iou, nms_class_aware, params)
    if nms is None:
        raise ValueError('dark_pred_tiled needs nms_iou: overlapping windows see the same sign more than once by construction')
    tiles.check_capacity(params.n_grid, params.n_boxes, query('cy_nms_max_per_image'))
    _restore(model, model_dir, params, restore_file)
    n = len(images)
    bs = max(_chunk_size(n, batch_size) // tiles.n_tiles, 1)            # the detector's batch stays near batch_size tiles
    side = int(params.darknet_input)
    idxs, xys, confs, clss, drawn = [], [], [], [], []
    model.eval()
    with torch.no_grad():
        for lo in range(0, n, bs):
            packed = PackedImages(images[lo:lo + bs], params.device)
            tables = [tiles.rects(int(h), int(w)) for h, w in packed.hw]
            tile_idx = np.concatenate([np.full(len(t), k, np.int32) for k, t in enumerate(tables)])
            tile_rect = np.concatenate(tables)
            y_hat = model(packed.crop_resize(tile_idx, tile_rect, side, side, 0.0, 1.0, True)).data
            _, idx, xy, cls, conf, _ = utils.decode_tiles_device(y_hat, params, tile_idx, tile_rect, packed.hw, 0.0, tiles.margin)
            _, idx, xy, conf, cls, _, _ = utils.nms_boxes_device(idx, xy, conf, cls, nms[0], nms[1], 0, packed.n)
            idx_np, xy_np, conf_np = idx.cpu().numpy().astype(np.int64), xy.cpu().numpy().reshape(-1, 4), conf.cpu().numpy()
            cls_np = cls.cpu().numpy().astype(np.int64) if cls is not None else None
            if draw:
                over = conf_np > np.float32(conf_th)
                d_idx, d_xy, d_cls = idx_np[over], xy_np[over], (cls_np[over] if cls_np is not None else None)
                colors = np.tile(np.array(box_draw.GREEN, dtype=np.uint8), (len(d_idx), 1))
                if y is not None:
                    _, t_idx, t_xy, t_cls = utils.decode_boxes_device(y[lo:lo + packed.n], params, packed.hw, conf_th)
                    d_idx = np.concatenate([d_idx, t_idx.cpu().numpy().astype(np.int64)])
                    d_xy = np.concatenate([d_xy, t_xy.cpu().numpy().reshape(-1, 4)])
                    if d_cls is not None:
                        d_cls = np.concatenate([d_cls, t_cls.cpu().numpy().astype(np.int64)])
                    colors = np.concatenate([colors, np.tile(np.array(box_draw.RED, dtype=np.uint8), (len(d_idx) - len(colors), 1))])
                drawn.extend(box_draw.unpack_images(box_draw.draw_boxes_device(packed, d_idx, d_xy, colors, d_cls), packed))
            idxs.append(idx_np + lo)
            xys.append(xy_np)
            confs.append(conf_np)
            clss.append(cls_np)
    merged = (np.concatenate(idxs), np.concatenate(xys, 0), np.concatenate(confs),
              np.concatenate(clss) if int(params.n_classes) else None)
    return merged, (drawn if draw else None)


def dark_class_pred(images, dark_model, dark_model_dir, dark_params, class_model, class_model_dir, class_params, restore_file,
                    batch_size=32, conf_th=0.5, draw=False, nms_iou=None, nms_class_aware=False):
    """predict_fns.py:75-82: detector -> crop of every box -> classifier -> utils.combine_y_hat.  Returns (y_hat float64 numpy
    [B, g, g, D + n_classes], None), or with draw=True (new, optional) (y_hat, images): the reference's second value, copies of
    the images with every box in green, labelled with the CLASSIFIER's argmax (predict_fns.py:80).  The classifier runs after the
    last detection chunk, so drawing walks the chunks a second time (upload, draw, download) and holds one chunk's images at a
    time; y_hat does not depend on it.  The crops are produced
    already centred ((v - 128) / 128, utils.center_rgb) in the classifier's NCHW layout and never leave the device.  No box over
    conf_th (new, optional; the reference's dark_pred default 0.5) is a valid outcome: the class part stays zero.
    nms_iou / nms_class_aware (new, optional): as in dark_pred -- the detector's y_hat is suppressed before the decode, so only the
    survivors are cropped, classified, combined and drawn, and the detector part of the returned y_hat is the masked one."""
    nms = _nms_option(nms_iou, nms_class_aware, dark_params)
    _restore(dark_model, dark_model_dir, dark_params, restore_file)
    _restore(class_model, class_model_dir, class_params, restore_file)
    ci = int(dark_params.capsule_input)
    dark_y_hat, crops, idx, xy = _detect_and_crop(images, dark_model, dark_params, conf_th, batch_size, ci, -128.0, 1.0 / 128.0, True, None, nms)
    n = int(crops.shape[0])
    n_classes = int(class_params.n_classes)
    class_model.eval()
    bs = max(int(batch_size) if batch_size else n, 1)
    scores = []
    with torch.no_grad():
        for lo in range(0, n, bs):
            scores.append(class_model(crops[lo:lo + bs]).data.reshape(-1, n_classes))
    class_y_hat = torch.cat(scores, 0) if scores else torch.zeros((0, n_classes), dtype=torch.float32, device=dark_y_hat.device)
    image_hw = np.array([np.asarray(im).shape[0:2] for im in images])
    y_hat = utils.combine_y_hat_device(image_hw, dark_y_hat, class_y_hat, idx, xy, dark_params)
    y_out = y_hat.cpu().numpy().astype(np.float64)
    if not draw:
        return y_out, None
    classes = np.argmax(class_y_hat.cpu().numpy(), axis=1).astype(np.int64) if n else np.zeros(0, np.int64)   # class_pred's argmax
    drawn = []
    bs = _chunk_size(len(images), batch_size)
    for lo in range(0, len(images), bs):
        packed = PackedImages(images[lo:lo + bs], dark_params.device)
        mine = (idx >= lo) & (idx < lo + packed.n)
        buf = box_draw.draw_boxes_device(packed, idx[mine] - lo, xy[mine], box_draw.GREEN, classes[mine])
        drawn.extend(box_draw.unpack_images(buf, packed))
    return y_out, drawn

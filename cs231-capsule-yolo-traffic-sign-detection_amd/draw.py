"""Boxes drawn on the device (the reference's plot.draw_boxes_vec, plot.py:5-64) into the packed image buffer of a chunk
(predict_fns.PackedImages), one launch of `cy_draw_boxes_u8` (csrc/draw.hip) for all boxes of the chunk.  DESIGN section 6g.

The outline is cv2.rectangle's thickness-1 rectangle as OpenCV documents it (both corners inclusive, clipped at the image); cv2 is
not a dependency, so that rule has NOT been compared with cv2.  The reference labels a box with `class_names[c]` in a Hershey font
(cv2.putText); neither the names file nor the font is available, so the label here is the class INDEX in decimal in the 5 x 7 font
below, its bottom-left corner at the reference's text origin ((x1 + x2) // 2, (y1 + y2) // 2).  Boxes are drawn in index order:
where two boxes of an image set the same pixel the later one wins, which is how a red ground-truth pass lands on a green prediction
pass.  There is no CPU fallback."""
import numpy as np
import torch

from ._lib import call

GREEN = (0, 255, 0)         # plot.py:5, the predictions (BGR like every image of the reference)
RED = (0, 0, 255)           # predict_fns.py:51, the ground truth

# digit -> 7 rows, top to bottom; bit 4 is the leftmost of the 5 columns.  The only copy: the kernel reads it through a pointer.
DIGITS_5X7 = np.array([
    [0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110],
    [0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110],
    [0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111],
    [0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110],
    [0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010],
    [0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110],
    [0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110],
    [0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000],
    [0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110],
    [0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100]], dtype=np.uint8)
LABEL_CELLS = (3 * 6 - 1) * 7      # the label block of up to three digits: 17 x 7 cells
COORD_LIMIT = 2 ** 30              # |corner| below this: x1 + x2 stays an int32

_glyphs = {}                       # device -> the uploaded table


def _glyphs_on(device):
    key = str(device)
    if key not in _glyphs:
        _glyphs[key] = torch.from_numpy(DIGITS_5X7.reshape(-1).copy()).to(device)
    return _glyphs[key]


def boxes_to_int(boxes_xy):
    """[n, 4] corners -> int32 with the reference's `xy[i].astype(int)` (plot.py:25): truncation towards zero.  ValueError on a
    corner that is not finite or whose magnitude reaches 2^30."""
    xy = np.asarray(boxes_xy)
    if xy.size == 0:
        return np.zeros((0, 4), dtype=np.int32)
    if xy.ndim != 2 or xy.shape[1] != 4:
        raise ValueError('boxes_xy must be [n, 4], got %s' % (xy.shape,))
    if xy.dtype.kind not in 'iu':
        xy = xy.astype(np.float64)
        if not np.all(np.isfinite(xy)):
            raise ValueError('box %d has a corner that is not finite' % int(np.argwhere(~np.isfinite(xy))[0, 0]))
        xy = np.trunc(xy)
    if np.any(np.abs(xy) >= COORD_LIMIT):
        raise ValueError('box %d has a corner of magnitude >= 2^30' % int(np.argwhere(np.abs(xy) >= COORD_LIMIT)[0, 0]))
    return np.ascontiguousarray(xy.astype(np.int32))


def draw_boxes_device(packed, box_img, boxes_xy, colors, labels=None):
    """plot.draw_boxes_vec on a PackedImages: a NEW uint8 device buffer laid out like packed.buf with the boxes drawn, box after box
    in the order given (packed.buf itself stays as it is: the crops are cut from the undrawn images, plot.py:22).  box_img [n]
    image indices, boxes_xy [n, 4] = (x1, y1, x2, y2) in pixels (float: truncated like astype(int)), colors one (b, g, r) or [n, 3],
    labels None or [n] integers (-1: no label, else 0..999, drawn as decimal digits).  ValueError: an image index outside the chunk,
    a label outside -1..999, a corner that is not finite or not below 2^30 in magnitude."""
    out = packed.buf.clone()
    idx = np.asarray(box_img, dtype=np.int64).reshape(-1)
    n = len(idx)
    xy = boxes_to_int(boxes_xy)
    col = np.asarray(colors)
    if col.ndim == 1:
        col = np.broadcast_to(col, (n, 3))
    if len(xy) != n or col.shape != (n, 3) or np.any(col < 0) or np.any(col > 255):
        raise ValueError('draw_boxes_device: %d image indices, %d boxes, colours %s' % (n, len(xy), col.shape))
    lab = None
    if labels is not None:
        lab = np.asarray(labels).reshape(-1)
        if len(lab) != n or (n and lab.dtype.kind not in 'iu'):
            raise ValueError('draw_boxes_device: labels %s %s for %d boxes' % (lab.dtype, lab.shape, n))
    if n == 0:
        return out
    idx = np.clip(idx, -1, np.iinfo(np.int32).max)                      # out of range stays out of range in 32 bits
    order = np.argsort(idx, kind='stable')                              # the boxes of an image contiguous, their order kept
    words = [idx[order].astype(np.int32), xy[order].reshape(-1)]
    if lab is not None:
        words.append(np.clip(lab[order], -2, 1000).astype(np.int32))
    words.append(np.zeros(1, dtype=np.int32))                           # the error word
    dev = out.device
    args = torch.from_numpy(np.concatenate(words)).to(dev)              # index, corners, [labels], error word: one upload
    cols = torch.from_numpy(np.ascontiguousarray(col[order].astype(np.uint8))).to(dev)
    max_items = 2 * int(packed.hw[:, 0].max() + packed.hw[:, 1].max()) + LABEL_CELLS
    base = args.data_ptr()
    call('cy_draw_boxes_u8', out.data_ptr(), packed.off.data_ptr(), packed.hw32.data_ptr(), packed.n, packed.nbytes,
         base, base + 4 * n, cols.data_ptr(), base + 20 * n if lab is not None else None, n, max_items,
         _glyphs_on(dev).data_ptr() if lab is not None else None, base + 4 * (len(args) - 1),
         torch.cuda.current_stream().cuda_stream)
    bad = int(args[-1].item())
    if bad:
        raise ValueError('draw_boxes_device: %d box(es) with an image index outside 0..%d or a label outside -1..999' % (bad, packed.n - 1))
    return out


def unpack_images(buf, packed):
    """A buffer laid out like packed.buf -> the list of its HWC uint8 images as numpy arrays (one device-to-host copy)."""
    host = buf.cpu().numpy()
    out, lo = [], 0
    for h, w in packed.hw:
        size = int(h) * int(w) * 3
        out.append(host[lo:lo + size].reshape(int(h), int(w), 3).copy())
        lo += size
    return out

"""numpy restatement of `cy_paste_resize_u8` (csrc/augment.hip) -- TEST INFRASTRUCTURE ONLY (nothing in the product imports this).

It does it the slow way: the composited frame is BUILT (pastes applied in order, each the sign's rectangle resized with the integer
rule to the destination's size), then its source rectangle is resized with the integer rule.  The kernel never forms that frame: it
asks, for each of an output pixel's four taps, which paste (if any) owns the tap, so equality of the two is a real cross-check.

  resize_int         the half-pixel bilinear rule in exact integers, round-half-up, uint8 -> uint8
  composite          the frame with a list of paste rows applied
  paste_resize_ref   every sample of one launch, uint8 [n, oh, ow, 3]
  center             (bytes - 128) / 128 as float32: what the two float output modes hold
"""
import numpy as np


def _taps(n_out, n_in):
    o = np.arange(n_out, dtype=np.int64)
    num = (2 * o + 1) * n_in - n_out
    r = num // (2 * n_out)                               # numpy's // is floor division
    return np.clip(r, 0, n_in - 1), np.clip(r + 1, 0, n_in - 1), num - r * 2 * n_out


def resize_int(image, oh, ow):
    """uint8 [h, w, 3] -> uint8 [oh, ow, 3]."""
    im = np.asarray(image).astype(np.int64)
    ra, rb, a = _taps(oh, im.shape[0])
    ca, cb, b = _taps(ow, im.shape[1])
    a, b = a[:, None, None], b[None, :, None]
    aa, ab, ba, bb = im[ra][:, ca], im[ra][:, cb], im[rb][:, ca], im[rb][:, cb]
    v = ((2 * ow - b) * (2 * oh - a) * aa + b * (2 * oh - a) * ab + (2 * ow - b) * a * ba + b * a * bb + 2 * ow * oh) // (4 * ow * oh)
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def composite(frame, signs, rows):
    """The frame (a copy) with the paste rows (sign, sy0, sy1, sx0, sx1, dy0, dy1, dx0, dx1) applied in order."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    for sg, sy0, sy1, sx0, sx1, dy0, dy1, dx0, dx1 in np.asarray(rows, dtype=np.int64).reshape(-1, 9):
        assert 0 <= dy0 < dy1 <= out.shape[0] and 0 <= dx0 < dx1 <= out.shape[1]
        out[dy0:dy1, dx0:dx1] = resize_int(signs[sg][sy0:sy1, sx0:sx1], dy1 - dy0, dx1 - dx0)
    return out


def paste_resize_ref(frames, signs, sample_img, sample_rect, begin, pastes, oh, ow):
    pastes = np.asarray(pastes, dtype=np.int64).reshape(-1, 9)
    out = np.empty((len(sample_img), oh, ow, 3), dtype=np.uint8)
    for s, img in enumerate(sample_img):
        y0, y1, x0, x1 = (int(v) for v in sample_rect[s])
        full = composite(frames[img], signs, pastes[begin[s]:begin[s + 1]])
        out[s] = resize_int(full[y0:y1, x0:x1], oh, ow)
    return out


def center(u8):
    return (u8.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)

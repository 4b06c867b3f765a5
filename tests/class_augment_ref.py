"""float64 numpy restatement of `cy_gather_jitter_u8` (csrc/augment.hip) -- TEST INFRASTRUCTURE ONLY (nothing in the product imports
this).  The whole rule, the slow way: gather by sample number, shift with zero fill, lightness gain, centre, NHWC -> NCHW, labels."""
import numpy as np


def brighten(k, d):
    """k [..., 3] source bytes as float64, d the lightness increase on the 0..1 V scale -> k' on the byte scale:
    hsv_to_rgb(rgb_to_hsv(k / 256) + (0, 0, d)) * 256.  V = max(k) / 256 grows by d while hue and saturation stay, so every channel
    is scaled by (v + 256 d) / v; a black pixel has saturation 0 and becomes the grey 256 d."""
    k = np.asarray(k, dtype=np.float64)
    v = k.max(axis=-1, keepdims=True)
    add = 256.0 * float(d)
    with np.errstate(divide='ignore', invalid='ignore'):
        scaled = k * ((v + add) / v)
    return np.where(v > 0, scaled, add)


def class_augment_ref(set_u8, labels, shift, light, index, swap=False, flip=False):
    """(x float64 [B, 3, H, W], y int64 [B], number of bad sample numbers).  shift [n, 2] = (dy, dx) / light [n] per SAMPLE NUMBER, or
    None.  Output pixel (y, x) of batch entry b reads pixel (y - dy, x - dx) of image index[b]; off the image it is 0 on all three
    channels and not brightened.  A sample number outside the set gives zeros and label -1.
    swap / flip: deliberately WRONG conventions ((dx, dy) order; the shift's sign), for the tests that show a case can tell them."""
    set_u8 = np.asarray(set_u8)
    n, H, W, _ = set_u8.shape
    index = np.asarray(index).reshape(-1)
    x = np.zeros((len(index), 3, H, W))
    y = np.full(len(index), -1, dtype=np.int64)
    bad = 0
    for b, s in enumerate(index):
        s = int(s)
        if not 0 <= s < n:
            bad += 1
            continue
        y[b] = labels[s]
        dy, dx = (int(v) for v in shift[s]) if shift is not None else (0, 0)
        if swap:
            dy, dx = dx, dy
        if flip:
            dy, dx = -dy, -dx
        d = float(light[s]) if light is not None else 0.0
        for oy in range(H):
            for ox in range(W):
                sy, sx = oy - dy, ox - dx
                if 0 <= sy < H and 0 <= sx < W:
                    x[b, :, oy, ox] = (brighten(set_u8[s, sy, sx].astype(np.float64), d) - 128.0) / 128.0
    return x, y, bad

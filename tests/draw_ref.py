"""Sequential numpy restatement of box drawing -- TEST INFRASTRUCTURE ONLY (nothing in the product imports this).

The yardstick of tests/test_gpu_draw.py for `cy_draw_boxes_u8` (csrc/draw.hip): the reference's plot.draw_boxes (plot.py:24-33)
executed box after box in index order with plain loops.  cv2 is not available, so the rectangle is the rule the C header states
(OpenCV's documented thickness-1 rectangle: both corners inclusive, clipped at the image) and the label is the stated deviation, the
class index in the 5 x 7 digit font of capsyolo_amd.draw.DIGITS_5X7.  tests/test_draw_host.py pins it against pixel sets written
out by hand.
"""
import numpy as np


def _put(img, x, y, color):
    if 0 <= y < img.shape[0] and 0 <= x < img.shape[1]:
        img[y, x] = color


def draw_ref(images, box_img, xy_int, colors, labels, glyphs):
    """Copies of `images` (HWC uint8) with box b = (x1, y1, x2, y2) = xy_int[b] drawn into image box_img[b] in colors[b], then its
    label labels[b] (labels None or -1: none), for b = 0, 1, ... in this order: a later box overwrites an earlier one.  A box whose
    image index lies outside the list or whose label lies outside -1..999 is skipped (the kernel counts it and draws nothing)."""
    out = [np.array(im, copy=True) for im in images]
    for b in range(len(box_img)):
        k = int(box_img[b])
        lab = -1 if labels is None else int(labels[b])
        if not 0 <= k < len(out) or not -1 <= lab <= 999:
            continue
        img = out[k]
        H, W = img.shape[:2]
        x1, y1, x2, y2 = (int(v) for v in xy_int[b])
        color = np.asarray(colors[b], dtype=np.uint8)
        # the outline; the loops run over the part inside the image only (a box may be 2^30 wide)
        for x in range(max(min(x1, x2), 0), min(max(x1, x2), W - 1) + 1):
            _put(img, x, y1, color)
            _put(img, x, y2, color)
        for y in range(max(min(y1, y2), 0), min(max(y1, y2), H - 1) + 1):
            _put(img, x1, y, color)
            _put(img, x2, y, color)
        if lab >= 0:
            xc, yc = (x1 + x2) // 2, (y1 + y2) // 2                  # Python's floor division (plot.py:30-31)
            for k_digit, ch in enumerate(str(lab)):
                rows = glyphs[int(ch)]
                for r in range(7):
                    for c in range(5):
                        if (int(rows[r]) >> (4 - c)) & 1:
                            _put(img, xc + 6 * k_digit + c, yc - 6 + r, color)
    return out


def from_art(rows):
    """A boolean mask from rows of '.' and '#'."""
    return np.array([[ch == '#' for ch in row] for row in rows])

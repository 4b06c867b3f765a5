"""Tiled detection: the table of overlapping windows of a frame on which the detector runs at close to native scale.

The detector resizes what it is given to darknet_input; a sign of a 1360 x 800 frame is a few pixels wide after that.  A tiling of
rows x cols windows that overlap by `overlap` pixels shows the detector every sign about rows (cols) times larger; the boxes of all
windows are put back into the frame by `cy_yolo_decode_tiles_conf` (the rule is in include/capsyolo_hip.h) and the duplicates in
the overlaps are merged by `cy_nms_boxes`.  This module is the host side, numpy only: the table and the options.
"""
import collections
import re

import numpy as np


def _axis(L, n, ov, name):
    """(tile length, the n starts) along one axis of length L: t = ceil((L + (n - 1) ov) / n), start_r = (r (L - t)) // (n - 1)."""
    t = -((-(L + (n - 1) * ov)) // n)
    if not (0 <= ov < t <= L):
        raise ValueError('tile_rects: %d tiles with an overlap of %d along the %s of %d pixels give a tile of %d: need 0 <= overlap < '
                         'tile <= %s' % (n, ov, name, L, t, name))
    return t, [0 if n == 1 else (r * (L - t)) // (n - 1) for r in range(n)]


def tile_rects(H, W, rows, cols, overlap, full=False):
    """int32 [T, 4] = (y0, y1, x0, x1), half-open, row-major, all tiles of one size: the first tile of an axis starts at 0, the last
    ends at the frame's edge, neighbours overlap by at least `overlap` pixels.  full: one more view, the whole frame (0, H, 0, W),
    for the signs that are larger than the overlap."""
    for name, v in (('H', H), ('W', W), ('rows', rows), ('cols', cols), ('overlap', overlap)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError('tile_rects: %s must be an integer, got %r' % (name, v))
    H, W, rows, cols, ov = int(H), int(W), int(rows), int(cols), int(overlap)
    if rows < 1 or cols < 1:
        raise ValueError('tile_rects: rows and cols must be >= 1, got %d x %d' % (rows, cols))
    th, ys = _axis(H, rows, ov, 'height')
    tw, xs = _axis(W, cols, ov, 'width')
    rects = [(y, y + th, x, x + tw) for y in ys for x in xs]
    if full:
        rects.append((0, H, 0, W))
    return np.array(rects, dtype=np.int32).reshape(-1, 4)


class TileSpec(collections.namedtuple('TileSpec', 'rows cols overlap full margin')):
    """The options of a tiling: rows x cols windows overlapping by `overlap` pixels, `full`: the whole frame as one more view,
    `margin`: the border rule's width in tile pixels (a box closer than that to a window edge inside the frame is left to the
    neighbouring window; negative: no border rule)."""
    __slots__ = ()

    def __new__(cls, rows, cols, overlap, full=False, margin=2.0):
        for name, v in (('rows', rows), ('cols', cols), ('overlap', overlap)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError('TileSpec: %s must be an integer, got %r' % (name, v))
        if rows < 1 or cols < 1 or overlap < 0:
            raise ValueError('TileSpec: rows, cols >= 1 and overlap >= 0, got %r x %r overlap %r' % (rows, cols, overlap))
        margin = float(margin)
        if margin != margin:
            raise ValueError('TileSpec: margin is not a number')
        return super(TileSpec, cls).__new__(cls, int(rows), int(cols), int(overlap), bool(full), margin)

    @property
    def n_tiles(self):
        return self.rows * self.cols + int(self.full)

    def rects(self, H, W):
        return tile_rects(H, W, self.rows, self.cols, self.overlap, self.full)

    def check_capacity(self, n_grid, n_boxes, capacity):
        """T g^2 n_boxes candidates of one frame must fit into the suppression step (capacity: cy_nms_max_per_image())."""
        per_frame = self.n_tiles * int(n_grid) * int(n_grid) * int(n_boxes)
        if per_frame > int(capacity):
            raise ValueError('%d tiles x %d x %d cells x %d boxes = %d candidates per frame, the suppression step holds %d'
                             % (self.n_tiles, n_grid, n_grid, n_boxes, per_frame, capacity))
        return per_frame


def parse_tiles(text):
    """'2x3' -> (2, 3): the command line's --tiles RxC."""
    m = re.match(r'^\s*(\d+)\s*[xX]\s*(\d+)\s*$', str(text))
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError('--tiles wants ROWSxCOLS with both >= 1, e.g. 2x3; got %r' % (text,))
    return int(m.group(1)), int(m.group(2))

"""Sign-paste augmentation of the detectors' data (the reference's build_data.py:171-288, `gtsdb_aug_`) and the resizes of the data-set
builder (build_data.py:44, 80), on the device through ONE kernel, `cy_paste_resize_u8` (csrc/augment.hip).  DESIGN section 6h.

The host plans (which sign goes where, and the label grid: a few numbers per box), the device does the pixels: an output sample is
the resized source rectangle of a frame with its pastes applied, computed without ever storing the composited frame.  Both resizes
follow INTER_LINEAR's half-pixel rule in exact integers with round-half-up (each yields a byte like cv2.resize does); cv2's 11-bit
fixed-point weights are not reproduced, and the reference's `random.choice(os.listdir(..))` stream cannot be: the randomness here is
`np.random.default_rng([seed, 17, sample, iteration])`, so a sample's plan depends on nothing else (not on the world size).

Rectangles are half-open (y0, y1, x0, x1); boxes are (x1, y1, x2, y2) like gt.txt.  A paste row is 9 ints: (sign, sy0, sy1, sx0, sx1,
dy0, dy1, dx0, dx1), the destination in full-frame coordinates.  There is no CPU fallback for the pixel work."""
import numpy as np
import torch

from ._lib import call, query

MAX_PASTES = 64                 # pastes per sample that the kernel stages (cy_paste_resize_max_pastes; tests hold the two equal)
MODES = {'u8': 0, 'f32_nhwc': 1, 'f32_nchw': 2}
RNG_STREAM = 17


class SignBank(object):
    """The signs that get pasted: `images` a list of uint8 [h, w, 3] arrays, `rois` [n, 4] = (y0, y1, x0, x1) inside each image (the
    GTSRB csv's Roi.Y1, Roi.Y2, Roi.X1, Roi.X2), `classes` [n].  The planning reads the host arrays only; `packed(device)` uploads
    the images once as a predict_fns.PackedImages."""

    def __init__(self, images, rois, classes):
        self.images = [np.ascontiguousarray(np.asarray(im)) for im in images]
        self.n = len(self.images)
        self.hw = np.array([im.shape[0:2] for im in self.images], dtype=np.int64).reshape(-1, 2)
        self.rois = np.asarray(rois, dtype=np.int64).reshape(-1, 4)
        self.classes = np.asarray(classes, dtype=np.int64).reshape(-1)
        if self.n == 0 or len(self.rois) != self.n or len(self.classes) != self.n:
            raise ValueError('SignBank: %d images, %d rois, %d classes' % (self.n, len(self.rois), len(self.classes)))
        y0, y1, x0, x1 = self.rois.T
        bad = (y0 < 0) | (y0 >= y1) | (y1 > self.hw[:, 0]) | (x0 < 0) | (x0 >= x1) | (x1 > self.hw[:, 1])
        if bad.any():
            raise ValueError('SignBank: the ROI of sign %d is empty or reaches outside its image' % int(np.argwhere(bad)[0, 0]))
        self._packed = {}

    def packed(self, device='cuda'):
        from .predict_fns import PackedImages
        key = str(device)
        if key not in self._packed:
            self._packed[key] = PackedImages(self.images, device)
        return self._packed[key]


def box_to_cell(box_xy, orig_hw, side, n_grid):
    """One box (x1, y1, x2, y2) of a frame of orig_hw through utils.resize_box_xy, xy_to_cwh and normalize_box_cwh (utils.py:174-230)
    for a side x side input and an n_grid x n_grid grid: the reference's double operations in its order, int() as truncation.
    Returns (resized_xy, cwh, normalized_cwh, (row, col)) like the three functions do."""
    orig_h, orig_w = float(orig_hw[0]), float(orig_hw[1])
    resized_h = resized_w = float(side)
    x1, y1, x2, y2 = (float(v) for v in box_xy)
    w_ratio = 1. * resized_w / orig_w                                  # resize_box_xy
    h_ratio = 1. * resized_h / orig_h
    rx1, rx2, ry1, ry2 = x1 * w_ratio, x2 * w_ratio, y1 * h_ratio, y2 * h_ratio
    xc, yc, bw, bh = (rx1 + rx2) / 2, (ry1 + ry2) / 2, rx2 - rx1, ry2 - ry1     # xy_to_cwh
    nw, nh = 1. * bw / resized_w, 1. * bh / resized_h                  # normalize_box_cwh
    grid_w, grid_h = 1. * resized_w / n_grid, 1. * resized_h / n_grid
    col, row = int(xc / grid_w), int(yc / grid_h)
    nxc, nyc = 1. * (xc - col * grid_w) / grid_w, 1. * (yc - row * grid_h) / grid_h
    return [rx1, ry1, rx2, ry2], [xc, yc, bw, bh], [nxc, nyc, nw, nh], (row, col)


def label_grid(boxes_xy, classes, orig_hw, side, n_grid, n_classes, skip_conflicts, conflicts=None):
    """float64 [g, g, 5 + C] of one frame: build_data.py:84-103 through resize_box_xy -> xy_to_cwh -> normalize_box_cwh
    (utils.py:174-230), the same double operations in the same order, int() as truncation.
    skip_conflicts=True (the plain build): a box whose cell is already taken is skipped, and its index is appended to the list
    `conflicts` when one is given.  skip_conflicts=False (the augmented samples, build_data.py:254-255, 279-280): a later box
    overwrites the cell's five numbers AND THE EARLIER CLASS BIT STAYS SET, so such a cell carries two class bits.  That is what the
    reference does; it is kept, not fixed.  ValueError for a box whose centre lies outside the grid (the reference raises IndexError
    or wraps around)."""
    g, C = int(n_grid), int(n_classes)
    y = np.zeros((g, g, 5 + C))
    for k, box in enumerate(np.asarray(boxes_xy, dtype=np.float64).reshape(-1, 4)):
        _, _, (nxc, nyc, nw, nh), (row, col) = box_to_cell(box, orig_hw, side, g)
        if not (0 <= row < g and 0 <= col < g):
            raise ValueError('box %d: its centre lies outside the %d x %d grid' % (k, g, g))
        if skip_conflicts and y[row, col, 0] == 1:
            if conflicts is not None:
                conflicts.append(k)
            continue
        y[row, col, 0:5] = [1, nxc, nyc, nw, nh]
        if C:
            c = int(classes[k])
            if not 0 <= c < C:
                raise ValueError('box %d: class %d outside 0..%d' % (k, c, C - 1))
            y[row, col, 5 + c] = 1
    return y


def sample_rng(seed, sample, iteration):
    return np.random.default_rng([int(seed), RNG_STREAM, int(sample), int(iteration)])


def plan_pastes(rng, boxes_xy, orig_hw, bank, add_signs):
    """The pastes of one augmented sample and its labels: (rows int32 [k, 9], boxes float64 [k, 4], classes int64 [k]) with
    k = n_boxes + add_signs.
    First one paste per existing box (build_data.py:231-257): a random sign's ROI resized into the box whose corners are truncated
    like `astype(int)`; the label is that truncated box with the SIGN's class.  Then add_signs pastes (build_data.py:260-280): a
    random sign's ROI copied 1:1 to (x, y) with x drawn from [0, W - sign width) and y from [0, H - sign height) -- the sizes of the
    whole sign IMAGE, as the reference draws them -- and the label box is the destination rectangle.  Per paste the generator is
    asked for the sign, then (additions) for x, then y.
    ValueError: a box whose truncated width or height is below 1 or that reaches outside the frame; a sign that does not fit.
    Two accidents of the reference are NOT reproduced: its `signs_list` is keyed by file name, so a sign drawn twice silently drops a
    paste; and it pastes into the frame in place, so the pastes of augmentation k leak into augmentation k + 1.  Here every
    augmented sample starts from the pristine frame and gets exactly n_boxes + add_signs pastes."""
    H, W = int(orig_hw[0]), int(orig_hw[1])
    rows, boxes, classes = [], [], []
    for k, box in enumerate(np.asarray(boxes_xy, dtype=np.float64).reshape(-1, 4)):
        if not np.all(np.isfinite(box)):
            raise ValueError('box %d has a corner that is not finite' % k)
        x1, y1, x2, y2 = (int(v) for v in box)
        if x2 - x1 < 1 or y2 - y1 < 1:
            raise ValueError('box %d is degenerate: %d x %d pixels after truncation' % (k, x2 - x1, y2 - y1))
        if x1 < 0 or y1 < 0 or x2 > W or y2 > H:
            raise ValueError('box %d reaches outside its %d x %d frame' % (k, H, W))
        s = int(rng.integers(0, bank.n))
        rows.append([s] + [int(v) for v in bank.rois[s]] + [y1, y2, x1, x2])
        boxes.append([x1, y1, x2, y2])
        classes.append(int(bank.classes[s]))
    for _ in range(int(add_signs)):
        s = int(rng.integers(0, bank.n))
        sh, sw = (int(v) for v in bank.hw[s])
        if W - sw < 1 or H - sh < 1:
            raise ValueError('sign %d (%d x %d) does not fit into the %d x %d frame' % (s, sh, sw, H, W))
        x = int(rng.integers(0, W - sw))
        y = int(rng.integers(0, H - sh))
        ry0, ry1, rx0, rx1 = (int(v) for v in bank.rois[s])
        rows.append([s, ry0, ry1, rx0, rx1, y, y + (ry1 - ry0), x, x + (rx1 - rx0)])
        boxes.append([x, y, x + (rx1 - rx0), y + (ry1 - ry0)])
        classes.append(int(bank.classes[s]))
    if len(rows) > MAX_PASTES:
        raise ValueError('%d pastes for one sample; the kernel stages at most %d' % (len(rows), MAX_PASTES))
    return (np.array(rows, dtype=np.int32).reshape(-1, 9), np.array(boxes, dtype=np.float64).reshape(-1, 4),
            np.array(classes, dtype=np.int64))


def full_rects(hw):
    """[n, 4] = (0, h, 0, w): the whole image as a source rectangle."""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    z = np.zeros(len(hw), np.int64)
    return np.stack([z, hw[:, 0], z, hw[:, 1]], axis=1)


def paste_resize_device(frames, bank, sample_img, sample_rect, begin, pastes, oh, ow, out='u8', into=None):
    """One launch of `cy_paste_resize_u8`.  frames: a predict_fns.PackedImages; bank: a SignBank (None when there are no pastes);
    sample_img [n], sample_rect [n, 4], begin [n + 1], pastes [k, 9].  out: 'u8' -> uint8 [n, oh, ow, 3]; 'f32_nhwc' -> float32
    [n, oh, ow, 3] and 'f32_nchw' -> float32 [n, 3, oh, ow], both (byte - 128) / 128.  into (optional): the tensor to write,
    of that shape and dtype.  ValueError when the kernel's error word is not zero (the samples it counts are zero-filled)."""
    if out not in MODES:
        raise ValueError('paste_resize_device: out is one of %s' % sorted(MODES))
    idx = np.ascontiguousarray(np.asarray(sample_img, dtype=np.int32).reshape(-1))
    rect = np.ascontiguousarray(np.asarray(sample_rect, dtype=np.int32).reshape(-1, 4))
    n = len(idx)
    beg = np.ascontiguousarray(np.asarray(begin if begin is not None else np.zeros(n + 1), dtype=np.int32).reshape(-1))
    rows = np.ascontiguousarray(np.asarray(pastes if pastes is not None else [], dtype=np.int32).reshape(-1, 9))
    if len(rect) != n or len(beg) != n + 1:
        raise ValueError('paste_resize_device: %d samples, %d rectangles, %d begin entries' % (n, len(rect), len(beg)))
    if len(rows) and bank is None:
        raise ValueError('paste_resize_device: %d pastes and no sign bank' % len(rows))
    oh, ow = int(oh), int(ow)
    dev = frames.buf.device
    shape = (n, 3, oh, ow) if out == 'f32_nchw' else (n, oh, ow, 3)
    dtype = torch.uint8 if out == 'u8' else torch.float32
    if into is None:
        into = torch.empty(shape, dtype=dtype, device=dev)
    elif tuple(into.shape) != shape or into.dtype != dtype or into.device != dev or not into.is_contiguous():
        raise ValueError('paste_resize_device: into must be a contiguous %s tensor %s on %s' % (dtype, shape, dev))
    if n == 0:
        return into
    signs = bank.packed(dev) if len(rows) else None
    args = torch.from_numpy(np.concatenate([idx, rect.reshape(-1), beg, rows.reshape(-1), [0]]).astype(np.int32)).to(dev)
    base = args.data_ptr()
    p_rect, p_beg, p_rows = base + 4 * n, base + 20 * n, base + 4 * (6 * n + 1)
    call('cy_paste_resize_u8', frames.buf.data_ptr(), frames.off.data_ptr(), frames.hw32.data_ptr(), frames.n, frames.nbytes,
         signs.buf.data_ptr() if signs else None, signs.off.data_ptr() if signs else None,
         signs.hw32.data_ptr() if signs else None, signs.n if signs else 0, signs.nbytes if signs else 0,
         base, p_rect, p_beg, n, p_rows if len(rows) else None, len(rows), oh, ow, MODES[out], into.data_ptr(),
         base + 4 * (len(args) - 1), torch.cuda.current_stream().cuda_stream)
    bad = int(args[-1].item())
    if bad:
        raise ValueError('paste_resize_device: %d sample(s) with an index, a rectangle or a paste slice out of range '
                         '(at most %d pastes per sample); they are zero-filled' % (bad, MAX_PASTES))
    return into


def window_labels(boxes_xy, classes, window, side, n_grid, n_classes, min_visible=0.6):
    """float64 [g, g, 5 + C]: the labels of one window (y0, y1, x0, x1), half-open, of a frame whose boxes are boxes_xy [k, 4] =
    (x1, y1, x2, y2) in frame pixels -- what a detector trained on the windows of a tiling (tiles.tile_rects) is to answer.  A box is
    labelled iff at least min_visible of its area lies inside the window; its label is the box clipped to the window, relative to
    the window's origin, through label_grid with the window's size as the image (skip_conflicts=False, as for every augmented
    sample).  A box without area is never labelled."""
    y0, y1, x0, x1 = (float(v) for v in window)
    kept, kept_classes = [], []
    for k, (bx1, by1, bx2, by2) in enumerate(np.asarray(boxes_xy, dtype=np.float64).reshape(-1, 4)):
        cx1, cy1, cx2, cy2 = max(bx1, x0), max(by1, y0), min(bx2, x1), min(by2, y1)
        area = (bx2 - bx1) * (by2 - by1)
        if not (area > 0 and cx2 > cx1 and cy2 > cy1):
            continue
        if (cx2 - cx1) * (cy2 - cy1) >= float(min_visible) * area:
            kept.append([cx1 - x0, cy1 - y0, cx2 - x0, cy2 - y0])
            kept_classes.append(classes[k] if n_classes else 0)
    return label_grid(np.array(kept, dtype=np.float64).reshape(-1, 4), kept_classes, (y1 - y0, x1 - x0), side, n_grid, n_classes,
                      skip_conflicts=False)


def plan_batch(frame_idx, hw, boxes, bank, add_signs, seed, iteration, side, n_grid, n_classes, tiles=None):
    """The plan of one batch of augmented samples.  frame_idx [n]: the numbers of the frames in the whole set, which seed the samples;
    hw [n, 2] and boxes (n arrays [k, 5]: x1, y1, x2, y2, class) belong to them in the same order.
    tiles (a tiles.TileSpec): every sample is ONE window of its frame's tile table, drawn after all paste draws of the sample -- so
    the pastes of a sample are the same with and without tiles -- and labelled by window_labels.  None: the whole frame, no draw.
    Returns (sample_rect [n, 4], begin [n + 1], pastes [k, 9], y float64 [n, g, g, 5 + C])."""
    begin, rows, ys, rects = [0], [], [], []
    for k, f in enumerate(frame_idx):
        b = np.asarray(boxes[k], dtype=np.float64).reshape(-1, 5)
        rng = sample_rng(seed, f, iteration)
        r, bx, cl = plan_pastes(rng, b[:, 0:4], hw[k], bank, add_signs)
        rows.append(r)
        begin.append(begin[-1] + len(r))
        if tiles is None:
            ys.append(label_grid(bx, cl, hw[k], side, n_grid, n_classes, skip_conflicts=False))
        else:
            table = tiles.rects(int(hw[k][0]), int(hw[k][1]))
            rects.append(table[int(rng.integers(0, len(table)))])
            ys.append(window_labels(bx, cl, rects[-1], side, n_grid, n_classes))
    pastes = np.concatenate(rows) if rows else np.zeros((0, 9), np.int32)
    sample_rect = full_rects(hw) if tiles is None else np.array(rects, dtype=np.int64).reshape(-1, 4)
    return sample_rect, np.array(begin, np.int32), pastes, np.stack(ys)


class AugmentFeeder(object):
    """The on-line form of the reference's `--aug N` copies: fresh pastes for every batch, made on the device between two steps.
    Iterates (x float32 NCHW centred, y float64) on the device like input_pipeline.DeviceFeeder, over `batches`, a list of arrays of
    frame numbers into `frames` (a predict_fns.PackedImages of the raw frames, resident on the device) and `boxes` (per frame a
    [k, 5] array x1, y1, x2, y2, class).  Per batch: the plan on the host, one upload of it, one launch.  Sample f of this feeder
    is seeded by (seed, f, iteration) with iteration = epoch * aug_stride + k, so every epoch sees new pastes and a given
    (seed, epoch) repeats exactly, whatever the batching or the number of ranks.
    tiles (a tiles.TileSpec): every sample is one randomly drawn window of its frame's tile table instead of the whole frame
    (plan_batch), so a detector can be trained on what serve.SignDetector(tiles=) will show it."""

    def __init__(self, frames, boxes, bank, batches, side, n_grid, n_classes, add_signs=0, seed=0, epoch=0, aug_stride=1, k=0, tiles=None):
        if not torch.cuda.is_available():
            from ._lib import HipExtensionError
            raise HipExtensionError('AugmentFeeder needs a GPU: the product path has no CPU fallback')
        self.frames, self.boxes, self.bank = frames, boxes, bank
        self.batches = [np.asarray(b, dtype=np.int64).reshape(-1) for b in batches]
        self.side, self.n_grid, self.n_classes, self.add_signs = int(side), int(n_grid), int(n_classes), int(add_signs)
        self.seed, self.iteration = int(seed), int(epoch) * int(aug_stride) + int(k)
        self.tiles = tiles

    def plan(self, frame_idx):
        idx = np.asarray(frame_idx, dtype=np.int64).reshape(-1)
        return plan_batch(idx, self.frames.hw[idx], [self.boxes[i] for i in idx], self.bank, self.add_signs, self.seed,
                          self.iteration, self.side, self.n_grid, self.n_classes, self.tiles)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        dev = self.frames.buf.device
        for idx in self.batches:
            rect, begin, pastes, y = self.plan(idx)
            x = paste_resize_device(self.frames, self.bank, idx, rect, begin, pastes, self.side, self.side, 'f32_nchw')
            yield x, torch.from_numpy(y).to(dev)


class AugmentSource(object):
    """What `main.py --augment` keeps between the epochs: the raw frames packed on the device, their boxes, the bank, and the epoch
    count.  feeder(batches) is the AugmentFeeder of the next epoch."""

    def __init__(self, frames, boxes, bank, side, n_grid, n_classes, add_signs, seed, device='cuda', tiles=None):
        from .predict_fns import PackedImages
        self.frames = PackedImages(frames, device)
        self.boxes = [np.asarray(b, dtype=np.float64).reshape(-1, 5) for b in boxes]
        if len(self.boxes) != self.frames.n:
            raise ValueError('AugmentSource: %d frames, %d box arrays' % (self.frames.n, len(self.boxes)))
        self.bank, self.args, self.seed, self.epoch = bank, (side, n_grid, n_classes, add_signs), seed, 0
        self.tiles = tiles
        bank.packed(device)

    def feeder(self, batches):
        f = AugmentFeeder(self.frames, self.boxes, self.bank, batches, *self.args, seed=self.seed, epoch=self.epoch, tiles=self.tiles)
        self.epoch += 1
        return f


def kernel_max_pastes():
    return int(query('cy_paste_resize_max_pastes'))

"""Synthetic GTSRB / GTSDB-shaped data (the reference ships none, .gitignore:1); shapes and dtypes of
what build_data.py emits.  Sample n is generated identically for every world size
so that data-parallel shards union to the single-process dataset."""
import numpy as np


def images(n, hw, seed=1234, first=0):
    """uint8 U{0..255} NHWC -> (x-128)/128 float32 (utils.py:122-123). Sample i depends only on (seed, first+i)."""
    out = np.empty((n, hw, hw, 3), dtype=np.float32)
    for i in range(n):
        rng = np.random.default_rng([seed, first + i])
        out[i] = (rng.integers(0, 256, (hw, hw, 3), dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    return out


def gtsrb_labels(n, n_classes=43, seed=1234, first=0):
    return np.array([np.random.default_rng([seed, 7, first + i]).integers(0, n_classes) for i in range(n)],
                    dtype=np.int64)


def gtsdb_labels(n, g, n_classes, seed=1234, first=0):
    """float64 [n,g,g,5+C]: 1..3 object cells per image: [1, xc, yc, w, h] + one-hot class (build_data.py:84-103)."""
    y = np.zeros((n, g, g, 5 + n_classes), dtype=np.float64)
    for i in range(n):
        rng = np.random.default_rng([seed, 11, first + i])
        k = min(int(rng.integers(1, 4)), g * g)
        for c in rng.choice(g * g, size=k, replace=False):
            r, col = divmod(int(c), g)
            y[i, r, col, 0] = 1.0
            y[i, r, col, 1:3] = rng.uniform(0.0, 1.0, 2)
            y[i, r, col, 3:5] = rng.uniform(0.02, 0.15, 2)
            if n_classes > 0:
                y[i, r, col, 5 + int(rng.integers(0, n_classes))] = 1.0
    return y


def raw_images(n, seed=1234, first=0, min_side=48, max_side=160):
    """A list of n uint8 HWC images of DIFFERENT sizes (min_side .. max_side per side), the shape of what predict mode reads
    from the raw GTSDB folder (main.py:305-306): a smooth gradient plus noise.  Image i depends only on (seed, first + i)."""
    out = []
    for i in range(n):
        rng = np.random.default_rng([seed, 13, first + i])
        h, w = (int(v) for v in rng.integers(min_side, max_side + 1, 2))
        ramp = np.add.outer(np.linspace(0, 96, h), np.linspace(0, 96, w))[:, :, None]
        out.append(np.clip(ramp + rng.integers(0, 64, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def sign_sequence(n, H=120, W=160, seed=1234, n_signs=3):
    """n uint8 HWC frames of ONE size from one camera: the background of raw_images (gradient plus noise, the same in every frame)
    and n_signs signs that drift at a constant velocity of up to 3 pixels a frame and grow by a pixel every other frame -- what a
    tracker has to follow.  A sign is a noise patch of 12 .. 20 pixels per side at frame 0, nearest-neighbour scaled to its size in
    the frame and clipped at the border.  The sequence depends only on (n_signs, H, W, seed); a longer one begins with the shorter."""
    rng = np.random.default_rng([seed, 17])
    ramp = np.add.outer(np.linspace(0, 96, H), np.linspace(0, 96, W))[:, :, None]
    back = np.clip(ramp + rng.integers(0, 64, (H, W, 3)), 0, 255).astype(np.uint8)
    signs = []
    for _ in range(n_signs):
        side = int(rng.integers(12, 21))
        signs.append(dict(patch=rng.integers(0, 256, (side, side, 3), dtype=np.uint8), side=side,
                          pos=rng.uniform([0.0, 0.0], [W - side, H - side]), vel=rng.uniform(-3.0, 3.0, 2)))
    out = []
    for i in range(n):
        frame = back.copy()
        for s in signs:
            side = s['side'] + i // 2
            x0, y0 = (int(v) for v in np.floor(s['pos'] + i * s['vel']))
            ys, xs = np.arange(y0, y0 + side), np.arange(x0, x0 + side)
            ky, kx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            if ky.any() and kx.any():
                src = (np.arange(side) * s['side']) // side
                frame[np.ix_(ys[ky], xs[kx])] = s['patch'][np.ix_(src[ky], src[kx])]
        out.append(frame)
    return out


def raw_boxes(images, n_classes=43, seed=1234, first=0):
    """Per image a float64 [k, 5] array (x1, y1, x2, y2, class), k = 1..3, the shape of the gt.txt rows of a GTSDB frame: boxes of
    8 .. a third of the shorter side, wholly inside the image, with fractional corners (so the truncation of the paste plan is
    exercised).  The boxes of image i depend only on (seed, first + i) and the image's size."""
    out = []
    for i, im in enumerate(images):
        h, w = np.asarray(im).shape[0:2]
        rng = np.random.default_rng([seed, 15, first + i])
        rows = []
        for _ in range(int(rng.integers(1, 4))):
            bw, bh = (int(v) for v in rng.integers(8, max(min(h, w) // 3, 9) + 1, 2))
            x1, y1 = float(rng.uniform(0, w - bw - 1)), float(rng.uniform(0, h - bh - 1))
            rows.append([x1, y1, x1 + bw, y1 + bh, float(rng.integers(0, max(n_classes, 1)))])
        out.append(np.array(rows, dtype=np.float64))
    return out


def sign_bank(n, n_classes=43, seed=1234):
    """(images, rois, classes) of n GTSRB-shaped signs: uint8 images of 12 .. 32 pixels per side, the ROI (y0, y1, x0, x1) 1 .. 3
    pixels inside the border like the csv's Roi columns, a class each.  Sign i depends only on (seed, i)."""
    images, rois, classes = [], [], []
    for i in range(n):
        rng = np.random.default_rng([seed, 16, i])
        h, w = (int(v) for v in rng.integers(12, 33, 2))
        m = [int(v) for v in rng.integers(1, 4, 4)]
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        rois.append([m[0], h - m[1], m[2], w - m[3]])
        classes.append(int(rng.integers(0, max(n_classes, 1))))
    return images, np.array(rois, dtype=np.int64), np.array(classes, dtype=np.int64)

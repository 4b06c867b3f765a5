"""The data-set builder (the reference's build_data.py:16-169) with every pixel on the device: frames and sign crops are resized,
and the `--aug N` copies composited, by `cy_paste_resize_u8` in chunks (augment.paste_resize_device).  No cv2: PPM is read by
interpret.read_ppm, and gt.txt and the GTSRB csv files are plain text.  JPEG input is not read.

    gtsdb(params, aug_size, root)   <root>/raw_GTSDB/{*.ppm, gt.txt[, Readme.txt]} -> <root>/{train,eval,test}.p, test_images.npy,
                                    class_names.txt (and train_raw.p with keep_raw)
    gtsrb(root)                     <root>/Images/<class>/{GT-<class>.csv, *.ppm} -> <root>/{train,eval,test}.p

What differs from the reference, on purpose: the resize rule (exact integers with round-half-up instead of cv2's 11-bit fixed-point
weights); the frames are taken in sorted file order and shuffled by np.random.RandomState(seed) (the reference
shuffles os.listdir order with the global numpy state); the augmentation's randomness and its two accidents (augment.plan_pastes)."""
import os
import pickle

import numpy as np
import torch

from . import augment, config
from .interpret import read_ppm
from .predict_fns import PackedImages

CHUNK = 32                     # frames per launch (32 frames of 800 x 1360 are 104 MB on the device)
SIGN_CHUNK = 4096              # GTSRB crops per launch


def _need_gpu():
    if not torch.cuda.is_available():
        raise SystemExit('build_data runs on hand-written gfx950 kernels only; no GPU is visible')


def read_gt(path):
    """gt.txt (`name;x1;y1;x2;y2;class` per line) -> {name: float64 [k, 5]} in file order."""
    out = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(';')
            if len(parts) != 6:
                raise ValueError('%s:%d: expected name;x1;y1;x2;y2;class' % (path, ln))
            out.setdefault(parts[0], []).append([float(v) for v in parts[1:5]] + [float(int(parts[5]))])
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


def read_sign_csv(path):
    """GT-<class>.csv (header, then `Filename;Width;Height;Roi.X1;Roi.Y1;Roi.X2;Roi.Y2;ClassId`) -> (names, rois int64 [n, 4] as
    (y0, y1, x0, x1) -- the crop im[Y1:Y2, X1:X2] of build_data.py:28-29 --, classes int64 [n], sizes int64 [n, 2] = (height, width))."""
    names, rois, classes, sizes = [], [], [], []
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    for ln, line in enumerate(lines[1:], 2):
        p = line.split(';')
        if len(p) != 8:
            raise ValueError('%s:%d: expected 8 fields' % (path, ln))
        w, h, x1, y1, x2, y2, c = (int(v) for v in p[1:8])
        names.append(p[0])
        rois.append([y1, y2, x1, x2])
        classes.append(c)
        sizes.append([h, w])
    return (names, np.array(rois, dtype=np.int64).reshape(-1, 4), np.array(classes, dtype=np.int64),
            np.array(sizes, dtype=np.int64).reshape(-1, 2))


def class_dirs(root):
    base = os.path.join(root, 'Images')
    return [d for d in sorted(os.listdir(base)) if len(d) == 5 and d.isdigit() and os.path.isdir(os.path.join(base, d))]


def read_gtsrb(root):
    """Every sign of <root>/Images/<class>/: (images, rois, classes, first), first[c] the index of class directory c's first sign."""
    images, rois, classes, first = [], [], [], [0]
    for d in class_dirs(root):
        prefix = os.path.join(root, 'Images', d)
        names, r, c, sizes = read_sign_csv(os.path.join(prefix, 'GT-' + d + '.csv'))
        for k, name in enumerate(names):
            im = read_ppm(os.path.join(prefix, name))
            if tuple(im.shape[0:2]) != tuple(sizes[k]):
                raise ValueError('%s/%s is %s, its csv row says %s' % (prefix, name, im.shape[0:2], tuple(sizes[k])))
            images.append(im)
        rois.append(r)
        classes.append(c)
        first.append(len(images))
    if not images:
        raise ValueError('no signs under %s/Images' % root)
    return images, np.concatenate(rois), np.concatenate(classes), first


def load_bank(root):
    images, rois, classes, _ = read_gtsrb(root)
    return augment.SignBank(images, rois, classes)


def read_class_names(path):
    """build_data.py:159-161: the lines of Readme.txt behind the 39th, the text after '='."""
    with open(path) as f:
        lines = [ln.strip() for ln in f.read().split('\n')[39:] if ln.strip()]
    return [ln.split('=')[1] for ln in lines if '=' in ln]


def _center64(u8):
    return (u8.astype(np.float64) - 128.0) / 128


def _composited_raw(frames, bank, begin, pastes, device):
    """The composited frames themselves: the kernel at each frame's own size, where the integer rule is the identity."""
    out = []
    packed = PackedImages(frames, device)
    for s, im in enumerate(frames):
        h, w = im.shape[0:2]
        rows = pastes[begin[s]:begin[s + 1]]
        u8 = augment.paste_resize_device(packed, bank, [s], [[0, h, 0, w]], [0, len(rows)], rows, h, w, 'u8')
        out.append(u8[0].cpu().numpy())
    return out


def gtsdb(params, aug_size=0, root=config.GTSDB, gtsrb_root=config.GTSRB, seed=0, keep_raw=False, device='cuda'):
    """build_data.py:63-169.  Returns a dict of what it wrote and counted (the plans of the augmented samples included, for tests)."""
    _need_gpu()
    aug_size = int(aug_size)
    side, g, C = int(params.darknet_input), int(params.n_grid), int(params.n_classes)
    add_signs = int(getattr(params, 'add_signs', 0))
    data_dir = os.path.join(root, 'raw_GTSDB')
    files = sorted(f for f in os.listdir(data_dir) if f.endswith('.ppm'))
    N = len(files)
    if N == 0:
        raise SystemExit('no .ppm frames under %s' % data_dir)
    gt = read_gt(os.path.join(data_dir, 'gt.txt'))
    bank = load_bank(gtsrb_root) if aug_size > 0 else None
    empty = np.zeros((0, 5))
    boxes = [gt.get(name, empty) for name in files]
    X = np.empty((N, side, side, 3), np.uint8)
    Y = np.empty((N, g, g, 5 + C))
    X_aug = np.empty((N * aug_size, side, side, 3), np.uint8)
    Y_aug = np.empty((N * aug_size, g, g, 5 + C))
    plans = [None] * (N * aug_size)
    conflicts = []
    for lo in range(0, N, CHUNK):
        frames = [read_ppm(os.path.join(data_dir, f)) for f in files[lo:lo + CHUNK]]
        packed = PackedImages(frames, device)
        n = packed.n
        X[lo:lo + n] = augment.paste_resize_device(packed, None, np.arange(n), augment.full_rects(packed.hw), None, None,
                                                   side, side, 'u8').cpu().numpy()
        for k in range(n):
            b = boxes[lo + k]
            Y[lo + k] = augment.label_grid(b[:, 0:4], b[:, 4], packed.hw[k], side, g, C, True, conflicts)
        for itr in range(aug_size):
            rect, begin, pastes, y = augment.plan_batch(np.arange(lo, lo + n), packed.hw, boxes[lo:lo + n], bank, add_signs, seed,
                                                        itr, side, g, C)
            x = augment.paste_resize_device(packed, bank, np.arange(n), rect, begin, pastes, side, side, 'u8').cpu().numpy()
            for k in range(n):
                j = (lo + k) * aug_size + itr                            # sample-major like the reference's X_aug
                X_aug[j], Y_aug[j] = x[k], y[k]
                plans[j] = pastes[begin[k]:begin[k + 1]].copy()
    perm = np.random.RandomState(seed).permutation(N)                    # utils.shuffle_aug: ONE permutation for both sets
    X, Y = X[perm], Y[perm]
    aug_perm = (perm[:, None] * aug_size + np.arange(aug_size)[None, :]).reshape(-1)
    X_aug, Y_aug = X_aug[aug_perm], Y_aug[aug_perm]
    print('Augmentation shape:')
    print(X_aug.shape)
    print(Y_aug.shape)
    split, split_aug = N // 10, N * aug_size // 10
    parts = {'eval': (slice(0, split), slice(0, split_aug)), 'test': (slice(split, 2 * split), slice(split_aug, 2 * split_aug)),
             'train': (slice(2 * split, None), slice(2 * split_aug, None))}
    shapes = {}
    for name, (sl, sl_aug) in parts.items():
        x, y = X[sl], Y[sl]
        if aug_size > 0:
            x, y = np.concatenate((x, X_aug[sl_aug]), axis=0), np.concatenate((y, Y_aug[sl_aug]), axis=0)
        with open(os.path.join(root, name + '.p'), 'wb') as f:
            pickle.dump((_center64(x), y), f, protocol=4)
        shapes[name] = (x.shape, y.shape)
    # the raw frames behind test.p, in its order: what `main.py --mode predict / detect` read next to it
    test_files = [files[i] for i in perm[split:2 * split]]
    test_raw = [read_ppm(os.path.join(data_dir, f)) for f in test_files]
    if aug_size > 0:
        for j in aug_perm[split_aug:2 * split_aug]:
            frame = read_ppm(os.path.join(data_dir, files[j // aug_size]))
            test_raw += _composited_raw([frame], bank, [0, len(plans[j])], plans[j], device)
    arr = np.empty(len(test_raw), dtype=object)
    for i, im in enumerate(test_raw):
        arr[i] = im
    np.save(os.path.join(root, 'test_images.npy'), arr, allow_pickle=True)
    if keep_raw:
        train_idx = perm[2 * split:]
        with open(os.path.join(root, 'train_raw.p'), 'wb') as f:
            pickle.dump(([read_ppm(os.path.join(data_dir, files[i])) for i in train_idx], [boxes[i] for i in train_idx]), f,
                        protocol=4)
    readme = os.path.join(data_dir, 'Readme.txt')
    if os.path.exists(readme):
        with open(os.path.join(root, 'class_names.txt'), 'w') as f:
            f.write(''.join(name + '\n' for name in read_class_names(readme)))
    n_boxes = int(sum(len(b) for b in gt.values()))
    print('Build dataset done.')
    print('Train shape:', *shapes['train'])
    print('Val shape:', *shapes['eval'])
    print('Test shape:', *shapes['test'])
    print('Number of boxes:', n_boxes)
    print('Conflict count:', len(conflicts))
    return {'files': files, 'perm': perm, 'aug_perm': aug_perm, 'plans': plans, 'boxes': boxes, 'shapes': shapes,
            'n_boxes': n_boxes, 'conflicts': len(conflicts)}


def gtsrb(root=config.GTSRB, seed=0, device='cuda'):
    """build_data.py:16-60: ROI crop -> 32 x 32 -> centred float32, split 10 % / 10 % / 80 % per class after a shuffle of the
    class, each part shuffled once more.  The kernel runs with empty paste slices."""
    _need_gpu()
    images, rois, classes, first = read_gtsrb(root)
    n = len(images)
    x = np.empty((n, 32, 32, 3), np.float32)
    for lo in range(0, n, SIGN_CHUNK):
        packed = PackedImages(images[lo:lo + SIGN_CHUNK], device)
        x[lo:lo + packed.n] = augment.paste_resize_device(packed, None, np.arange(packed.n), rois[lo:lo + packed.n], None, None,
                                                          32, 32, 'f32_nhwc').cpu().numpy()
    rs = np.random.RandomState(seed)
    idx = {'eval': [], 'test': [], 'train': []}
    for c in range(len(first) - 1):
        members = first[c] + rs.permutation(first[c + 1] - first[c])
        split = len(members) // 10
        idx['eval'].append(members[:split])
        idx['test'].append(members[split:2 * split])
        idx['train'].append(members[2 * split:])
    shapes = {}
    for name in ('train', 'eval', 'test'):
        i = np.concatenate(idx[name])
        i = i[rs.permutation(len(i))]
        with open(os.path.join(root, name + '.p'), 'wb') as f:
            pickle.dump((x[i], classes[i]), f, protocol=4)
        shapes[name] = (x[i].shape, classes[i].shape)
    print('Train shape:', *shapes['train'])
    print('Val shape:', *shapes['eval'])
    print('Test shape:', *shapes['test'])
    return shapes

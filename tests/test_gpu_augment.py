"""`cy_paste_resize_u8` (csrc/augment.hip) and everything built on it, on the GPU: the fused composite-and-resize against the slow
restatement tests/augment_ref.py BIT FOR BIT (the kernel never forms the composited frame, the yardstick does), its error word, the
data-set builder end to end on files written here, and the on-line path (AugmentFeeder, main.py --augment)."""
import importlib.util
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

from helpers import REPO

from capsyolo_amd import augment, build_data, interpret, synth, utils
from capsyolo_amd.predict_fns import PackedImages
from augment_ref import center, composite, paste_resize_ref, resize_int

pytestmark = pytest.mark.gpu

FRAME_SIZES = [(37, 53), (64, 48), (48, 48), (90, 33), (33, 90)]
SIGN_SIZES = [(9, 7), (12, 15), (20, 18), (25, 31), (33, 24), (40, 31)]
SIGN_ROIS = [(1, 8, 1, 6), (1, 11, 2, 14), (2, 18, 1, 16), (2, 23, 3, 29), (1, 31, 2, 22), (2, 38, 1, 30)]


def _scene():
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in FRAME_SIZES]
    signs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIGN_SIZES]
    return frames, augment.SignBank(signs, SIGN_ROIS, np.arange(6))


def _row(bank, s, dy0, dy1, dx0, dx1):
    return [s] + [int(v) for v in bank.rois[s]] + [dy0, dy1, dx0, dx1]


def _samples(bank):
    """(sample_img, sample_rect, begin, pastes) of the parity case: one sample per situation."""
    one_to_one = _row(bank, 1, 80, 90, 21, 33)                        # ROI 10 x 12 copied 1:1, touching the bottom-right corner of 90 x 33
    assert one_to_one[2] - one_to_one[1] == 10 and one_to_one[4] - one_to_one[3] == 12
    per_sample = [
        (0, (0, 37, 0, 53), []),                                       # no paste
        (1, (0, 64, 0, 48), [_row(bank, 5, 10, 28, 5, 20)]),           # destination 18 x 15 smaller than the ROI 36 x 29
        (2, (0, 48, 0, 48), [_row(bank, 0, 5, 45, 8, 40)]),            # destination 40 x 32 larger than the ROI 7 x 5
        (3, (0, 90, 0, 33), [one_to_one]),
        (4, (0, 33, 0, 90), [_row(bank, 2, 2, 22, 10, 40), _row(bank, 3, 10, 30, 30, 70), _row(bank, 4, 5, 28, 35, 50)]),   # overlapping: order matters
        (1, (8, 50, 3, 30), [_row(bank, 3, 20, 60, 10, 44)]),          # a proper crop that cuts through the paste
    ]
    idx = [s[0] for s in per_sample]
    rect = [s[1] for s in per_sample]
    begin = np.concatenate([[0], np.cumsum([len(s[2]) for s in per_sample])])
    pastes = np.array([r for s in per_sample for r in s[2]], dtype=np.int32)
    return idx, rect, begin, pastes


@pytest.mark.parametrize('oh,ow', [(32, 32), (96, 96), (40, 56)])
def test_composite_parity_bit_for_bit(oh, ow):
    frames, bank = _scene()
    idx, rect, begin, pastes = _samples(bank)
    want = paste_resize_ref(frames, bank.images, idx, rect, begin, pastes, oh, ow)
    # the overlapping sample depends on the order of its pastes, so the case can tell a wrong order
    flipped = pastes.copy()
    flipped[[3, 5]] = pastes[[5, 3]]                                   # rows 3..5 are sample 4's
    assert not np.array_equal(paste_resize_ref(frames, bank.images, idx, rect, begin, flipped, oh, ow)[4], want[4])
    packed = PackedImages(frames)
    got = augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, oh, ow, 'u8')
    assert got.dtype == torch.uint8 and tuple(got.shape) == (6, oh, ow, 3)
    got = got.cpu().numpy()
    for s in range(6):
        assert np.array_equal(got[s], want[s]), 'sample %d: %d bytes differ' % (s, int((got[s] != want[s]).sum()))
    nhwc = augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, oh, ow, 'f32_nhwc')
    nchw = augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, oh, ow, 'f32_nchw')
    assert nhwc.dtype == nchw.dtype == torch.float32 and tuple(nchw.shape) == (6, 3, oh, ow)
    assert np.array_equal(nhwc.cpu().numpy(), center(want))
    assert np.array_equal(nchw.cpu().numpy(), center(want).transpose(0, 3, 1, 2))


def test_taps_that_straddle_the_edge_of_a_paste():
    frames = [np.zeros((40, 40, 3), np.uint8)]
    bank = augment.SignBank([np.full((10, 10, 3), 255, np.uint8)], [(1, 9, 1, 9)], [0])
    pastes = [[0, 1, 9, 1, 9, 13, 21, 17, 25]]                        # 8 x 8, copied 1:1
    want = paste_resize_ref(frames, bank.images, [0], [(0, 40, 0, 40)], [0, 1], pastes, 25, 25)
    got = augment.paste_resize_device(PackedImages(frames), bank, [0], [(0, 40, 0, 40)], [0, 1], pastes, 25, 25, 'u8').cpu().numpy()
    assert np.array_equal(got, want)
    assert ((got > 0) & (got < 255)).any() and (got == 255).any() and (got == 0).any()      # blends of inside and outside taps


def _bad_cases(bank):
    """name -> (begin, pastes, the bad sample, the good one).  Sample 0 reads frame 1 (64 x 48), sample 1 frame 2 (48 x 48)."""
    good = _row(bank, 3, 4, 30, 6, 40)
    cap = augment.MAX_PASTES
    return {
        'sign index n_signs': ([0, 1, 2], [[bank.n] + good[1:], good], 0, 1),
        'destination one pixel past the frame': ([0, 1, 2], [good, _row(bank, 3, 20, 49, 6, 40)], 1, 0),
        'ROI outside its sign': ([0, 1, 2], [[3, 2, 26, 3, 29, 4, 30, 6, 40], good], 0, 1),            # sign 3 is 25 rows high
        'decreasing begin': ([2, 1, 2], [good, good], 0, 1),
        'one paste more than the cap': ([0, cap + 1, cap + 2], [_row(bank, 0, 1, 8, 1, 6)] * (cap + 1) + [good], 0, 1),
    }


@pytest.mark.parametrize('name', ['sign index n_signs', 'destination one pixel past the frame', 'ROI outside its sign',
                                  'decreasing begin', 'one paste more than the cap'])
@pytest.mark.parametrize('mode', ['u8', 'f32_nchw'])
def test_error_word(name, mode):
    frames, bank = _scene()
    begin, pastes, bad, good = _bad_cases(bank)[name]
    idx, rect = [1, 2], [(0, 64, 0, 48), (0, 48, 0, 48)]
    shape, dtype = ((2, 24, 24, 3), torch.uint8) if mode == 'u8' else ((2, 3, 24, 24), torch.float32)
    into = torch.full(shape, 77, dtype=dtype, device='cuda')
    with pytest.raises(ValueError, match='1 sample'):
        augment.paste_resize_device(PackedImages(frames), bank, idx, rect, begin, pastes, 24, 24, mode, into=into)
    got = into.cpu().numpy()
    assert not got[bad].any()                                          # zero-filled
    want = paste_resize_ref(frames, bank.images, [idx[good]], [rect[good]], [begin[good], begin[good + 1]], pastes, 24, 24)[0]
    assert np.array_equal(got[good], want if mode == 'u8' else center(want).transpose(2, 0, 1))
    assert want.any()


def test_exactly_the_cap_is_accepted_and_empty_launches():
    frames, bank = _scene()
    cap = augment.MAX_PASTES
    pastes = [_row(bank, k % 6, 1 + k % 5, 20 + k % 7, 2 + k % 3, 30 + k % 11) for k in range(cap)]
    want = paste_resize_ref(frames, bank.images, [2], [(0, 48, 0, 48)], [0, cap], pastes, 24, 24)
    packed = PackedImages(frames)
    got = augment.paste_resize_device(packed, bank, [2], [(0, 48, 0, 48)], [0, cap], pastes, 24, 24, 'u8').cpu().numpy()
    assert np.array_equal(got, want)
    assert tuple(augment.paste_resize_device(packed, None, [], np.zeros((0, 4)), [0], None, 8, 8, 'u8').shape) == (0, 8, 8, 3)
    plain = augment.paste_resize_device(packed, None, [0], [(0, 37, 0, 53)], None, None, 37, 53, 'u8').cpu().numpy()
    assert np.array_equal(plain[0], frames[0])                        # equal size: the identity


# ---------------------------------------------------------------------------------------------- the builder, end to end

def _write_trees(tmp_path):
    gtsdb_root, gtsrb_root = tmp_path / 'GTSDB', tmp_path / 'GTSRB'
    raw = gtsdb_root / 'raw_GTSDB'
    raw.mkdir(parents=True)
    frames = synth.raw_images(12, min_side=48, max_side=96)
    boxes = [np.trunc(b) for b in synth.raw_boxes(frames)]             # gt.txt holds integers
    boxes[5] = np.zeros((0, 5))                                        # a frame without a sign
    lines = []
    for i, (im, b) in enumerate(zip(frames, boxes)):
        interpret.write_ppm(str(raw / ('%05d.ppm' % i)), im)
        lines += ['%05d.ppm;%d;%d;%d;%d;%d' % ((i,) + tuple(int(v) for v in row)) for row in b]
    (raw / 'gt.txt').write_text('\n'.join(lines) + '\n')
    (raw / 'Readme.txt').write_text('\n'.join(['.'] * 39 + ['%d = name %d' % (c, c) for c in range(43)]) + '\n')
    images, rois, _ = synth.sign_bank(12)
    for c in range(3):
        d = gtsrb_root / 'Images' / ('%05d' % c)
        d.mkdir(parents=True)
        rows = ['Filename;Width;Height;Roi.X1;Roi.Y1;Roi.X2;Roi.Y2;ClassId']
        for k in range(4):
            im, (y0, y1, x0, x1) = images[4 * c + k], rois[4 * c + k]
            interpret.write_ppm(str(d / ('%05d_%05d.ppm' % (k, c))), im)
            rows.append('%05d_%05d.ppm;%d;%d;%d;%d;%d;%d;%d' % (k, c, im.shape[1], im.shape[0], x0, y0, x1, y1, c))
        (d / ('GT-%05d.csv' % c)).write_text('\n'.join(rows) + '\n')
    return str(gtsdb_root), str(gtsrb_root), frames, boxes, images, rois


def test_builder_end_to_end(tmp_path):
    root, sroot, frames, boxes, signs, rois = _write_trees(tmp_path)
    params = types.SimpleNamespace(darknet_input=64, n_grid=2, n_classes=43, add_signs=1)
    res = build_data.gtsdb(params, aug_size=2, root=root, gtsrb_root=sroot, seed=3, keep_raw=True)
    assert sorted(os.listdir(root)) == ['class_names.txt', 'eval.p', 'raw_GTSDB', 'test.p', 'test_images.npy', 'train.p', 'train_raw.p']
    parts = {name: pickle.load(open(os.path.join(root, name + '.p'), 'rb')) for name in ('train', 'eval', 'test')}
    for name, n in (('train', 10 + 20), ('eval', 1 + 2), ('test', 1 + 2)):      # 12 frames: split 1, and 24 copies: split 2
        X, Y = parts[name]
        assert X.shape == (n, 64, 64, 3) and X.dtype == np.float64 and Y.shape == (n, 2, 2, 48) and Y.dtype == np.float64
        k = X * 128 + 128
        assert np.array_equal(k, np.rint(k)) and k.min() >= 0 and k.max() <= 255          # every value is k / 128 - 1
    assert res['n_boxes'] == sum(len(b) for b in boxes) and res['files'] == ['%05d.ppm' % i for i in range(12)]
    perm, aug_perm = res['perm'], res['aug_perm']
    assert sorted(perm) == list(range(12)) and aug_perm.tolist() == [2 * p + k for p in perm for k in (0, 1)]
    bank = augment.SignBank(signs, rois, np.repeat(np.arange(3), 4))
    # one plain sample: the first of eval.p is frame perm[0]
    f = int(perm[0])
    X, Y = parts['eval']
    assert np.array_equal(X[0], (resize_int(frames[f], 64, 64).astype(np.float64) - 128) / 128)
    assert np.array_equal(Y[0], augment.label_grid(boxes[f][:, 0:4], boxes[f][:, 4], frames[f].shape, 64, 2, 43, True))
    # one augmented sample: the second of eval.p is copy aug_perm[0], recomputed from its own seed through the yardstick
    j = int(aug_perm[0])
    f, itr = j // 2, j % 2
    rows, lab, cls = augment.plan_pastes(augment.sample_rng(3, f, itr), boxes[f][:, 0:4], frames[f].shape, bank, 1)
    assert len(rows) == len(boxes[f]) + 1 and np.array_equal(rows, res['plans'][j])
    full = composite(frames[f], signs, rows)
    assert np.array_equal(X[1], (resize_int(full, 64, 64).astype(np.float64) - 128) / 128)
    assert np.array_equal(Y[1], augment.label_grid(lab, cls, frames[f].shape, 64, 2, 43, False))
    # test_images.npy: the raw frames behind test.p in its order, the augmented ones composited
    raw = list(np.load(os.path.join(root, 'test_images.npy'), allow_pickle=True))
    assert len(raw) == 3 and raw[0].dtype == np.uint8 and np.array_equal(raw[0], frames[int(perm[1])])
    for im, j in zip(raw[1:], aug_perm[2:4]):
        assert np.array_equal(im, composite(frames[int(j) // 2], signs, res['plans'][int(j)]))
    Xt = parts['test'][0]
    assert np.array_equal(Xt[2], (resize_int(raw[2], 64, 64).astype(np.float64) - 128) / 128)
    raw_frames, raw_boxes = pickle.load(open(os.path.join(root, 'train_raw.p'), 'rb'))
    assert len(raw_frames) == 10 and all(np.array_equal(a, frames[int(i)]) for a, i in zip(raw_frames, perm[2:]))
    assert all(np.array_equal(a, boxes[int(i)]) for a, i in zip(raw_boxes, perm[2:]))
    assert open(os.path.join(root, 'class_names.txt')).read().split('\n')[:2] == [' name 0', ' name 1']
    x_tr, y_tr, x_ev, y_ev = utils.load_data(root)
    assert x_tr.shape == (30, 64, 64, 3) and y_ev.shape == (3, 2, 2, 48)
    # the classifier sets: 4 signs per class -> split 0, so all 12 land in train.p (10 % / 10 % / 80 % of 4, rounded down)
    shapes = build_data.gtsrb(sroot, seed=3)
    x, y = pickle.load(open(os.path.join(sroot, 'train.p'), 'rb'))
    assert x.shape == (12, 32, 32, 3) and x.dtype == np.float32 and sorted(y.tolist()) == [0] * 4 + [1] * 4 + [2] * 4
    for name in ('eval', 'test'):
        xe, ye = pickle.load(open(os.path.join(sroot, name + '.p'), 'rb'))
        assert xe.shape == (0, 32, 32, 3) and xe.dtype == np.float32 and ye.shape == (0,)
    assert shapes['train'] == ((12, 32, 32, 3), (12,))
    want = {center(resize_int(im[y0:y1, x0:x1], 32, 32)).tobytes(): c for im, (y0, y1, x0, x1), c in zip(signs, rois, np.repeat(np.arange(3), 4))}
    assert len(want) == 12 and all(want.get(x[i].tobytes()) == y[i] for i in range(12))
    x_tr, y_tr, x_ev, y_ev = utils.load_data(sroot)
    assert x_tr.shape == (12, 32, 32, 3) and x_ev.shape == (0, 32, 32, 3)


def test_gtsrb_split_sizes_with_ten_per_class(tmp_path):
    """Classes of 10 and 23 signs: 1 / 1 / 8 and 2 / 2 / 19."""
    images, rois, _ = synth.sign_bank(33)
    lo = 0
    for c, n in enumerate((10, 23)):
        d = tmp_path / 'Images' / ('%05d' % c)
        d.mkdir(parents=True)
        rows = ['Filename;Width;Height;Roi.X1;Roi.Y1;Roi.X2;Roi.Y2;ClassId']
        for k in range(n):
            im, (y0, y1, x0, x1) = images[lo + k], rois[lo + k]
            interpret.write_ppm(str(d / ('%05d.ppm' % k)), im)
            rows.append('%05d.ppm;%d;%d;%d;%d;%d;%d;%d' % (k, im.shape[1], im.shape[0], x0, y0, x1, y1, c))
        (d / ('GT-%05d.csv' % c)).write_text('\n'.join(rows) + '\n')
        lo += n
    shapes = build_data.gtsrb(str(tmp_path))
    assert [shapes[k][0][0] for k in ('eval', 'test', 'train')] == [3, 3, 27]
    _, y = pickle.load(open(str(tmp_path / 'train.p'), 'rb'))
    assert sorted(y.tolist()) == [0] * 8 + [1] * 19


# ---------------------------------------------------------------------------------------------- the on-line path

def test_augment_feeder_repeats_per_seed_and_epoch():
    frames = synth.raw_images(8)
    boxes = synth.raw_boxes(frames)
    bank = augment.SignBank(*synth.sign_bank(6))
    packed = PackedImages(frames)
    batches = [np.array([5, 2, 7, 0]), np.array([1, 3, 6, 4])]
    mk = lambda seed, epoch: augment.AugmentFeeder(packed, boxes, bank, batches, 64, 2, 43, add_signs=2, seed=seed, epoch=epoch)
    run = lambda feeder: [(x.clone(), y.clone()) for x, y in feeder]
    a, b, c, d = run(mk(1, 0)), run(mk(1, 0)), run(mk(1, 1)), run(mk(2, 0))
    assert len(mk(1, 0)) == 2 and len(a) == 2
    for (xa, ya), (xb, yb) in zip(a, b):
        assert xa.dtype == torch.float32 and tuple(xa.shape) == (4, 3, 64, 64) and xa.is_cuda
        assert ya.dtype == torch.float64 and tuple(ya.shape) == (4, 2, 2, 48) and ya.is_cuda
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert not torch.equal(a[0][0], c[0][0]) and not torch.equal(a[0][0], d[0][0])
    feeder = mk(1, 0)
    for (xa, ya), idx in zip(a, batches):
        rect, begin, pastes, y = feeder.plan(idx)
        assert len(pastes) == sum(len(boxes[i]) for i in idx) + 2 * 4
        assert torch.equal(xa, augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, 64, 64, 'f32_nchw'))
        assert np.array_equal(ya.cpu().numpy(), y)
        want = paste_resize_ref(frames, bank.images, idx, rect, begin, pastes, 64, 64)
        assert np.array_equal(xa.cpu().numpy(), center(want).transpose(0, 3, 1, 2))
    # a sample does not depend on the batch it travels in (so not on the number of ranks)
    solo = next(iter(augment.AugmentFeeder(packed, boxes, bank, [np.array([7])], 64, 2, 43, add_signs=2, seed=1, epoch=0)))
    assert torch.equal(solo[0][0], a[0][0][2])


def test_main_trains_with_and_without_augment(tmp_path):
    mdir = str(tmp_path / 'darknet_d')
    os.makedirs(mdir)
    json.dump(dict(batch_size=4, n_epochs=1, lr_decay=0.5, l_coord=5, l_noobj=0.5, n_boxes=2, n_classes=0, n_grid=2, darknet_input=64,
                   capsule_input=32, dropout=0.0, add_signs=1), open(os.path.join(mdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_augment', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    argv = ['--model', 'darknet_d', '--synthetic', '8', '--n_epochs', '1', '--batch_size', '4', '--no_metric', '--model_dir', mdir]
    losses_tr, losses_ev = m.main(argv + ['--augment'])
    assert len(losses_tr) == 1 and np.isfinite(losses_tr[0]) and np.isfinite(losses_ev[0])
    plain_tr, plain_ev = m.main(argv)
    assert len(plain_tr) == 1 and np.isfinite(plain_tr[0]) and np.isfinite(plain_ev[0])
    with pytest.raises(SystemExit):
        m.main(argv + ['--augment', '--graph'])
    with pytest.raises(SystemExit):
        m.main(['--model', 'capsule', '--synthetic', '8', '--augment', '--model_dir', mdir])

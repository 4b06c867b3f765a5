"""`cy_gather_jitter_u8` (csrc/augment.hip) and everything built on it, on the GPU: the kernel against the float64 restatement
tests/class_augment_ref.py (bit for bit where the lightness is 0, within 1e-6 on the centred scale where it is not: three fp32
roundings of a value below 268 byte units, 4.8e-5, times 1/128, plus the subtraction's 2^-18 / 128 -- about 4e-7), its identity with
`cy_center_u8` at zero jitter, its error word, the feeder, and `main.py --class_augment`."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO

from capsyolo_amd import _lib, class_augment, synth
from capsyolo_amd.input_pipeline import DeviceFeeder
from class_augment_ref import class_augment_ref

pytestmark = pytest.mark.gpu

H, W = 12, 10                                                        # not square, W no multiple of 4, less than one 256-pixel tile
SHIFTS = [(0, 0), (4, -4), (-4, 4), (11, 0), (0, -9), (12, 3), (0, 0)]          # per sample number; (12, 3) is wholly off the image
LIGHTS = [0.0, 0.05, 0.0371, 0.05, 0.0, 0.05, 0.0371]


def _small_set():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (7, H, W, 3), dtype=np.uint8)
    x[1] = 0                                                         # all black: v = 0, the grey 256 d
    x[2] = 255
    x[6, :, :, 1] = 0                                                # a zero channel stays zero
    x[4, 0, 0] = 0                                                   # one black pixel among others
    return x, np.array([5, 0, 42, 7, 7, 19, 3], dtype=np.int64)


def _launch(x, labels, shift, light, index, prefill=None):
    """One launch through the C-ABI: (x_out, y_out, error word) as numpy."""
    dev = 'cuda'
    set_d, lab_d = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    sh_d = torch.from_numpy(np.ascontiguousarray(shift, dtype=np.int32)).to(dev) if shift is not None else None
    li_d = torch.from_numpy(np.ascontiguousarray(light, dtype=np.float32)).to(dev) if light is not None else None
    idx_d = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(dev)
    B = len(index)
    out = torch.full((B, 3) + x.shape[1:3], 77.0 if prefill is None else prefill, dtype=torch.float32, device=dev)
    y = torch.full((B,), 77, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call('cy_gather_jitter_u8', set_d.data_ptr(), lab_d.data_ptr(), len(x), x.shape[1], x.shape[2],
              sh_d.data_ptr() if sh_d is not None else None, li_d.data_ptr() if li_d is not None else None, idx_d.data_ptr(), B,
              out.data_ptr(), y.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), y.cpu().numpy(), int(err.item())


def _center(x_u8, index):
    """cy_center_u8 on the gathered bytes: float32 NCHW."""
    g = torch.from_numpy(np.ascontiguousarray(x_u8[np.asarray(index)])).cuda()
    B, h, w, _ = g.shape
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device='cuda')
    _lib.call('cy_center_u8', g.data_ptr(), out.data_ptr(), B, h, w, 3, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_parity_with_the_restatement():
    x, labels = _small_set()
    index = [3, 0, 5, 1, 4, 2]
    shift, light = np.array(SHIFTS, dtype=np.int32), np.array(LIGHTS, dtype=np.float32)
    # every listed shift and every listed lightness, each lightness also on an unshifted and on the black / white image
    cases = [(index, shift, light),
             ([6, 2, 2, 1, 0, 4], np.roll(shift, 3, axis=0), np.roll(light, 1)),        # a repeated sample number
             ([0, 1, 2, 4, 5, 6], None, np.array([0.05, 0.05, 0.0371, 0.0371, 0.0, 0.0, 0.05], dtype=np.float32))]
    for idx, sh, li in cases:
        want, want_y, bad = class_augment_ref(x, labels, sh, li, idx)
        assert bad == 0
        if sh is not None:                                           # the case can tell a wrong convention
            assert not np.array_equal(class_augment_ref(x, labels, sh, li, idx, swap=True)[0], want)
            assert not np.array_equal(class_augment_ref(x, labels, sh, li, idx, flip=True)[0], want)
        got, got_y, err = _launch(x, labels, sh, li, idx)
        assert err == 0 and np.array_equal(got_y, want_y) and np.array_equal(got_y, labels[idx])
        for b, s in enumerate(idx):
            if li[s] == 0:
                assert np.array_equal(got[b].astype(np.float64), want[b]), 'entry %d (sample %d): not bit-identical' % (b, s)
            else:
                diff = float(np.abs(got[b].astype(np.float64) - want[b]).max())
                print('entry %d sample %d shift %s light %.4f: max |diff| = %.3g' % (b, s, None if sh is None else sh[s].tolist(), li[s], diff))
                assert diff <= 1e-6, 'entry %d (sample %d): %g' % (b, s, diff)
        assert got.max() > 1.0 or 2 not in idx                       # white brightened passes 1: nothing is clipped
    # all six shifts were exercised, the wholly-off one gives an all-zero image although it is brightened
    got, _, _ = _launch(x, labels, shift, light, [5])
    assert not got.any() and LIGHTS[5] > 0 and SHIFTS[5] == (12, 3)


@pytest.mark.parametrize('shape', ['12x10', '32x32'])
def test_zero_jitter_is_cy_center_u8_bit_for_bit(shape):
    if shape == '12x10':
        x, labels = _small_set()
        index, batches = [3, 0, 5, 1, 4, 2], [[3, 0, 5, 1], [4, 2, 6]]
    else:
        x = np.random.default_rng(8).integers(0, 256, (64, 32, 32, 3), dtype=np.uint8)
        labels = np.arange(64, dtype=np.int64) % 43
        index = np.random.default_rng(9).permutation(64)
        batches = [index[:40], index[40:]]                           # 1024 pixels: four tiles per sample
    want = _center(x, index)
    n = len(x)
    for sh, li in ((None, None), (np.zeros((n, 2), np.int32), np.zeros(n, np.float32)), (None, np.zeros(n, np.float32))):
        got, y, err = _launch(x, labels, sh, li, index)
        assert err == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(y, labels[np.asarray(index)])
    src = class_augment.ClassAugmentSource(x, labels, seed=1, max_shift=0, max_light=0.0)
    mine = [(a.clone(), b.clone()) for a, b in src.feeder(batches)]
    theirs = [(a.clone(), b.clone()) for a, b in DeviceFeeder([(x[np.asarray(b)], labels[np.asarray(b)]) for b in batches], 'cuda')]
    assert len(mine) == len(theirs) == 2
    for (xa, ya), (xb, yb) in zip(mine, theirs):
        assert xa.dtype == xb.dtype == torch.float32 and xa.shape == xb.shape and ya.dtype == yb.dtype == torch.int64
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ya, yb)


def test_error_word_guards_bad_sample_numbers():
    x, labels = _small_set()
    shift, light = np.array(SHIFTS, dtype=np.int32), np.array(LIGHTS, dtype=np.float32)
    index = [3, -1, 0, 7, 4]                                          # -1 and n_set: never dereferenced
    want, want_y, bad = class_augment_ref(x, labels, shift, light, index)
    assert bad == 2 and want_y.tolist() == [7, -1, 5, -1, 7]
    got, y, err = _launch(x, labels, shift, light, index)
    assert err == 2 and np.array_equal(y, want_y)
    assert not got[1].any() and not got[3].any()
    for b in (0, 2, 4):
        assert np.abs(got[b].astype(np.float64) - want[b]).max() <= 1e-6 and got[b].any()
    assert np.array_equal(got[2].astype(np.float64), want[2])        # sample 0: no jitter
    src = class_augment.ClassAugmentSource(x, labels, seed=0)
    for bad_number in (-1, 7):
        with pytest.raises(ValueError, match='sample number %d ' % bad_number):
            src.feeder([[3, 0], [bad_number, 4]])


def test_feeder_repeats_per_seed_and_epoch_and_ignores_the_batching():
    x, labels = _small_set()
    batches = [np.array([5, 2, 6, 0]), np.array([1, 3, 4])]
    run = lambda feeder: [(a.clone(), b.clone()) for a, b in feeder]
    src = class_augment.ClassAugmentSource(x, labels, seed=1)
    f0 = src.feeder(batches)
    e0, e1 = run(f0), run(src.feeder(batches))
    again = run(class_augment.ClassAugmentSource(x, labels, seed=1).feeder(batches))
    other = run(class_augment.ClassAugmentSource(x, labels, seed=2).feeder(batches))
    assert len(f0) == 2 and len(e0) == 2 and src.epoch == 2
    for (xa, ya), (xb, yb), idx in zip(e0, again, batches):
        assert xa.dtype == torch.float32 and tuple(xa.shape) == (len(idx), 3, H, W) and xa.is_cuda
        assert ya.dtype == torch.int64 and np.array_equal(ya.cpu().numpy(), labels[idx])
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert not torch.equal(e0[0][0], e1[0][0]) and not torch.equal(e0[0][0], other[0][0])
    # the feeder's batches are the kernel on the feeder's own tables, which are jitter_tables(seed, epoch)
    shift, light = class_augment.jitter_tables(7, 1, 0)
    assert np.array_equal(f0.shift, shift) and np.array_equal(f0.light, light) and shift.any() and light.any()
    for (xa, _), idx in zip(e0, batches):
        want = class_augment_ref(x, labels, shift, light, idx)[0]
        assert np.abs(xa.cpu().numpy().astype(np.float64) - want).max() <= 1e-6
    # a sample does not depend on the batch it travels in (so not on the number of ranks)
    solo = run(class_augment.ClassAugmentSource(x, labels, seed=1).feeder([np.array([6])]))
    assert torch.equal(solo[0][0][0], e0[0][0][2])
    assert run(class_augment.ClassAugmentSource(x, labels, seed=1).feeder([])) == []


@pytest.mark.parametrize('graph', [False, True])
def test_main_trains_capsule_with_class_augment(tmp_path, graph):
    mdir = str(tmp_path / 'capsule')
    os.makedirs(mdir)
    params = json.load(open(os.path.join(REPO, 'experiments', 'capsule', 'params.json')))
    json.dump(params, open(os.path.join(mdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_class_augment', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    argv = ['--model', 'capsule', '--synthetic', '16', '--n_epochs', '2', '--batch_size', '8', '--no_metric', '--class_augment',
            '--model_dir', mdir] + (['--graph'] if graph else [])
    losses_tr, losses_ev = m.main(argv)
    assert len(losses_tr) == 2 and len(losses_ev) == 2 and np.all(np.isfinite(losses_tr)) and np.all(np.isfinite(losses_ev))

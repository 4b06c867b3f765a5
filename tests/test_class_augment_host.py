"""Host-side tests of the classifiers' augmentation (no GPU): the lightness rule of tests/class_augment_ref.py against what the
reference's own utils.augmentation returned (tests/golden/classaug.npz), the per-epoch jitter tables, the C-ABI's new symbol and
the new command-line flag."""
import importlib.util
import os
import re

import numpy as np
import pytest

from helpers import REPO, load_golden

from capsyolo_amd import _lib, augment, class_augment
from class_augment_ref import class_augment_ref


def _main_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------- the lightness rule against the reference

def test_lightness_rule_matches_the_reference():
    g = load_golden('classaug')
    x, d, out = g['x'], float(g['light']), g['out']
    assert x.dtype == np.float64 and out.dtype == np.float64 and x.shape == out.shape == (4, 8, 8, 3)
    k = x * 128.0 + 128.0
    assert np.array_equal(k, np.rint(k)) and k.min() == 0 and k.max() == 255
    k = k.astype(np.uint8)
    px = k.reshape(-1, 3)
    assert (px == 0).all(1).any() and (px == 255).all(1).any() and (px == 128).all(1).any()       # black, white, grey
    assert ((px == 0).sum(1) == 1).any()                                                          # one zero channel
    assert 0.04 < d < float(g['max_light'])
    got, y, bad = class_augment_ref(k, np.arange(4), None, np.full(4, d), np.arange(4))
    assert bad == 0 and y.tolist() == [0, 1, 2, 3]
    want = (2.0 * out - 1.0).transpose(0, 3, 1, 2)                    # the reference answers on the 0..1 scale, NHWC
    err = float(np.abs(got - want).max())
    print('restatement against the reference: max |diff| = %.3g' % err)
    assert err <= 1e-12
    assert want.max() > 1.0                                           # no clipping: a white pixel passes 1
    # the reference throws its shift away (it drew a non-zero one): its answer is that of the UNSHIFTED batch
    assert np.abs(g['shift_drawn']).min() > 0


def test_restatement_shift_convention_and_zero_fill():
    rng = np.random.default_rng(2)
    k = rng.integers(1, 256, (1, 5, 4, 3), dtype=np.uint8)
    x, _, _ = class_augment_ref(k, [7], np.array([[2, -1]]), None, [0])
    c = (k[0].astype(np.float64) - 128.0) / 128.0
    # shifted[max(0, h):h + H] = x[max(0, -h):-h + H] (utils.py:130-137): down by 2, left by 1
    assert np.array_equal(x[0, :, 2:, :3], c[:3, 1:].transpose(2, 0, 1))
    assert not x[0, :, :2, :].any() and not x[0, :, :, 3].any()
    assert not class_augment_ref(k, [7], np.array([[5, 0]]), np.array([0.05]), [0])[0].any()        # wholly off: zeros, not brightened
    x, y, bad = class_augment_ref(k, [7], None, None, [-1, 0, 1])
    assert bad == 2 and y.tolist() == [-1, 7, -1] and not x[0].any() and not x[2].any() and np.array_equal(x[1], c.transpose(2, 0, 1))


# ---------------------------------------------------------------- the tables

def test_jitter_tables():
    shift, light = class_augment.jitter_tables(4096, 3, 0, 4, 0.05)
    assert shift.dtype == np.int32 and shift.shape == (4096, 2) and light.dtype == np.float32 and light.shape == (4096,)
    assert shift.min() == -4 and shift.max() == 4
    assert sorted(np.unique(shift).tolist()) == list(range(-4, 5))
    assert light.min() >= 0 and light.max() < np.float32(0.05) and light.max() > 0.049
    again = class_augment.jitter_tables(4096, 3, 0, 4, 0.05)
    assert np.array_equal(shift, again[0]) and np.array_equal(light, again[1])
    for other in (class_augment.jitter_tables(4096, 3, 1, 4, 0.05), class_augment.jitter_tables(4096, 4, 0, 4, 0.05)):
        assert not np.array_equal(shift, other[0]) and not np.array_equal(light, other[1])
    shift, light = class_augment.jitter_tables(100, 3, 0, 0, 0.0)
    assert shift.dtype == np.int32 and shift.shape == (100, 2) and not shift.any()
    assert light.dtype == np.float32 and light.shape == (100,) and not light.any()
    shift, light = class_augment.jitter_tables(4096, 0, 5, 1, 1e-3)
    assert set(np.unique(shift).tolist()) == {-1, 0, 1} and 0 <= light.min() and light.max() < np.float32(1e-3)
    assert class_augment.RNG_STREAM != augment.RNG_STREAM
    with pytest.raises(ValueError):
        class_augment.jitter_tables(8, 0, 0, -1, 0.05)
    with pytest.raises(ValueError):
        class_augment.jitter_tables(8, 0, 0, 4, -0.1)


def test_tables_do_not_depend_on_the_batching():
    """Sample s of a set of n: its entry is row s of ONE draw over the set, so neither the batches nor the ranks can move it."""
    shift, light = class_augment.jitter_tables(64, 9, 2)
    rng = np.random.default_rng([9, class_augment.RNG_STREAM, 2])
    assert np.array_equal(shift, rng.integers(-4, 5, size=(64, 2)).astype(np.int32))


# ---------------------------------------------------------------- C-ABI and command line

def test_cabi_exports_the_gather_kernel():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    assert re.search(r'\bint\s+cy_gather_jitter_u8\s*\(', header)
    lib = _lib.load()
    assert 'cy_gather_jitter_u8' in _lib.EXPORTS and hasattr(lib, 'cy_gather_jitter_u8')
    assert len(_lib._SIGS['cy_gather_jitter_u8']) == 13
    _lib.call('cy_gather_jitter_u8', None, None, 1, 8, 8, None, None, None, 0, None, None, None, None)   # B = 0 is valid and launches nothing
    with pytest.raises(_lib.HipExtensionError, match='null argument'):
        _lib.call('cy_gather_jitter_u8', None, None, 1, 8, 8, None, None, None, 1, None, None, None, None)
    with pytest.raises(_lib.HipExtensionError, match='B = -1'):
        _lib.call('cy_gather_jitter_u8', None, None, 1, 8, 8, None, None, None, -1, None, None, None, None)
    for n_set, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -2)):           # sizes are refused before anything is launched
        with pytest.raises(_lib.HipExtensionError, match='a set of'):
            _lib.call('cy_gather_jitter_u8', 1, 1, n_set, H, W, None, None, 1, 1, 1, 1, 1, None)


def test_main_accepts_and_refuses_class_augment():
    m = _main_module('cy_main_class_augment_host')
    args = m.parser.parse_args(['--model', 'capsule', '--class_augment'])
    assert args.class_augment is True and m.parser.parse_args([]).class_augment is False
    assert callable(m.class_augmented_data) and '--class_augment' in m.__doc__ and 'aug_max_light' in m.__doc__
    tail = ['--synthetic', '8', '--n_epochs', '1', '--no_metric']
    with pytest.raises(SystemExit, match='class_augment'):
        m.main(['--model', 'darknet_d', '--class_augment'] + tail)
    with pytest.raises(SystemExit, match='give one'):
        m.main(['--model', 'darknet_d', '--augment', '--class_augment'] + tail)
    with pytest.raises(SystemExit, match='give one'):
        m.main(['--model', 'capsule', '--augment', '--class_augment'] + tail)
    with pytest.raises(SystemExit, match='class_augment'):
        m.main(['--model', 'capsule', '--mode', 'predict', '--restore', 'last', '--class_augment'] + tail)

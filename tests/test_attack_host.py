"""CPU-side tests of the image-gradient / attack feature: the numpy restatements of tests/attack_ref.py against torch's own autograd
and against the properties of the step rule, ops.image_grad_plan, the untouched conv_plan, main.py's refusals before any device
work, and the C ABI's new symbols."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attack_ref
from helpers import REPO

from capsyolo_amd import _lib, ops

F32 = np.float32


# ---------------------------------------------------------------- the restated image gradient
@pytest.mark.parametrize('B,H,W,Cout,k,pad', [(2, 12, 11, 5, 9, 0), (3, 7, 5, 4, 3, 1), (1, 6, 6, 3, 5, 2)])
def test_restated_image_gradient_equals_autograd(B, H, W, Cout, k, pad):
    rng = np.random.default_rng(7 + k)
    x = torch.from_numpy(rng.standard_normal((B, 3, H, W))).requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((Cout, 3, k, k)))
    z = F.conv2d(x, w, None, 1, pad)
    dy = torch.from_numpy(rng.standard_normal(tuple(z.shape)))                     # NCHW cotangent
    (want,) = torch.autograd.grad((z * dy).sum(), x)
    got, mag = attack_ref.image_grad(dy.permute(0, 2, 3, 1).numpy(), w.numpy(), H, W, pad)
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12 * float(mag.max()))
    # the activation's derivative and the BatchNorm scale on the loads: lrelu(conv(x) * scale + shift), act = the block's output
    scale = torch.from_numpy(rng.uniform(0.5, 2.0, Cout))
    shift = torch.from_numpy(rng.standard_normal(Cout))
    x2 = x.detach().clone().requires_grad_(True)
    out = F.leaky_relu(F.conv2d(x2, w, None, 1, pad) * scale[None, :, None, None] + shift[None, :, None, None], 0.01)
    (want2,) = torch.autograd.grad((out * dy).sum(), x2)
    got2, _ = attack_ref.image_grad(dy.permute(0, 2, 3, 1).numpy(), w.numpy(), H, W, pad, act=out.detach().permute(0, 2, 3, 1).numpy(),
                                    slope=0.01, scale=scale.numpy())
    np.testing.assert_allclose(got2, want2.numpy(), rtol=0, atol=1e-12 * float(mag.max()) * 2.0)


def test_restated_image_gradient_in_int64():
    rng = np.random.default_rng(3)
    dy, w = rng.integers(-2, 3, (2, 4, 4, 6)), rng.integers(-2, 3, (6, 3, 3, 3))
    gi, mag = attack_ref.image_grad(dy, w, 4, 4, 1, dtype=np.int64)
    gf, _ = attack_ref.image_grad(dy, w, 4, 4, 1)
    assert gi.dtype == np.int64 and np.array_equal(gi, gf) and np.all(np.abs(gi) <= mag)


# ---------------------------------------------------------------- the step rule
def test_step_rule_on_edge_values():
    inf, nan = np.inf, np.nan
    eps, alpha, lo, hi = F32(2 / 128), F32(1 / 128), F32(-1.0), F32(127 / 128)
    x0 = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5, -1.0, 127 / 128, 0.25, 0.25, -0.999, 0.99], dtype=F32)
    x = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.5 + 2 / 128, 0.5 - 2 / 128, -1.0, 127 / 128, 0.25, 0.25, -0.999, 0.99], dtype=F32)
    g = np.array([0.0, nan, inf, -inf, -0.0, 1.0, -1.0, -3.0, 5.0, 1e-30, -1e-30, -1.0, 1.0], dtype=F32)
    got = attack_ref.attack_step(x, x0, g, alpha, eps, lo, hi)
    assert got.dtype == F32
    # g = 0, -0 and NaN leave x alone; +-inf moves like any sign
    assert got[0] == 0 and got[1] == 0 and got[4] == 0 and got[2] == alpha and got[3] == -alpha
    # at the eps edge a further step is projected back; a step inwards is not
    assert got[5] == x[5] and got[6] == x[6]
    # at lo / hi the range clamp wins
    assert got[7] == lo and got[8] == hi and got[11] == lo and got[12] == hi
    # the smallest gradients still count as a sign
    assert got[9] == F32(0.25) + alpha and got[10] == F32(0.25) - alpha
    # properties on random values: inside the ball (up to the one rounding of the bound) and inside [lo, hi]; g = 0 with x inside is the identity
    rng = np.random.default_rng(0)
    x0 = ((rng.integers(0, 256, 4099).astype(F32) - 128) / 128).astype(F32)
    x = np.clip(x0 + rng.uniform(-2 / 128, 2 / 128, 4099).astype(F32), lo, hi).astype(F32)
    g = rng.standard_normal(4099).astype(F32)
    out = attack_ref.attack_step(x, x0, g, alpha, eps, lo, hi)
    assert np.all(out >= np.maximum(x0 - eps, lo)) and np.all(out <= np.minimum(x0 + eps, hi))
    moved = out - x
    assert np.all(moved * np.sign(g) >= 0)                    # never against the gradient's sign
    keep = attack_ref.attack_step(x, x0, np.zeros_like(g), alpha, eps, lo, hi)
    inside = (np.abs(x - x0) <= eps)
    assert np.array_equal(keep[inside], x[inside])
    # bytes stay bytes: on byte-exact images with eps, alpha whole grey levels every result is a whole grey level
    xb = attack_ref.attack_step(x0, x0, g, alpha, eps, lo, hi)
    assert np.array_equal(xb * 128, np.rint(xb * 128)) and np.all(np.abs(xb - x0) <= eps)


def test_saliency_rule():
    g = np.zeros((3, 3, 2, 2), dtype=F32)
    g[0, :, 0, 0] = [1, -4, 2]
    g[0, :, 0, 1] = [np.nan, 0.5, -2]
    g[0, :, 1, 0] = [0.0, 0.0, 0.0]
    g[0, :, 1, 1] = [np.nan, np.nan, np.nan]
    g[2, 0] = np.inf
    g[2, 1, 0, 0] = 1e30
    s = attack_ref.saliency_u8(g)
    assert s.dtype == np.uint8 and s.shape == (3, 2, 2)
    assert s[0].tolist() == [[255, 128], [0, 0]]               # 2 / 4 * 255 = 127.5 -> 128 (halves up)
    assert not s[1].any()                                      # an all-zero image
    assert (s[2] == 255).all()                                 # infinity counts as the largest finite float


# ---------------------------------------------------------------- the plan
def test_image_grad_plan_takes_the_three_first_layers():
    for shape, cout, k, pad in (((1024, 3, 32, 32), 256, 9, 0), ((64, 3, 32, 32), 64, 3, 1), ((2, 3, 416, 416), 32, 3, 1),
                                ((2, 3, 608, 608), 128, 3, 1), ((3, 3, 7, 5), 5, 3, 1), ((1, 3, 4, 4), 3, 1, 0)):
        p = ops.image_grad_plan(shape, cout, k, 1, pad)
        assert p.ok and p.family == 'conv_image_grad', (shape, cout, k, pad)
        B, _, H, W = shape
        assert p.tile == (16, 32) and p.blocks == B * -(-H // 16) * -(-W // 32) and p.chunks == -(-cout // 8)


@pytest.mark.parametrize('shape,cout,k,stride,pad', [
    ((2, 4, 32, 32), 64, 3, 1, 1),        # Cin != 3
    ((2, 1, 32, 32), 64, 3, 1, 1),
    ((2, 3, 32, 32), 64, 3, 2, 1),        # stride 2
    ((2, 3, 32, 32), 64, 4, 1, 1),        # even k
    ((2, 3, 32, 32), 64, 11, 1, 5),       # k > 9
    ((2, 3, 32, 32), 64, 3, 1, 2),        # pad > k // 2
    ((2, 3, 32, 32), 1025, 3, 1, 1),      # Cout > 1024
    ((2, 3, 32, 32), 0, 3, 1, 1),
    ((2, 3, 8, 32), 16, 9, 1, 0),         # H < k - 2 pad: the forward has no output
])
def test_image_grad_plan_refuses(shape, cout, k, stride, pad):
    p = ops.image_grad_plan(shape, cout, k, stride, pad)
    assert not p.ok and p.blocks == 0


def test_conv_plan_is_untouched():
    """Two rows of tests/test_conv_plan_host.py's table, and the field list: the image gradient has its own plan function."""
    assert ops.ConvPlan._fields == ('fwd', 'dgrad', 'wgrad', 'in_affine', 'dgrad_bn_fuse', 'dgrad_premasks', 'wgrad_bn', 'wgrad_bn4',
                                    'conv1', 'conv1_bwd', 'conv1_moments', 'conv1_onepass', 'conv1_signmask')
    p = ops.conv_plan((4, 3, 64, 64), 128, 3, 1, 1, nchw=True)
    assert (p.fwd, p.dgrad, p.wgrad, p.conv1) == ('conv1_fwd', None, 'conv1_wgrad', True)
    p = ops.conv_plan((8, 3, 32, 32), 256, 9, 1, 0, nchw=True, relu=True)
    assert (p.fwd, p.dgrad, p.wgrad, p.conv1) == ('conv_gemm_fwd', None, 'conv_wgrad', False)
    p = ops.conv_plan((4, 64, 64, 128), 256, 3, 1, 1)
    assert (p.fwd, p.dgrad, p.wgrad) == ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wino_wgrad')


# ---------------------------------------------------------------- main.py and the C ABI
def _main():
    spec = importlib.util.spec_from_file_location('cy_main_attack', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_attack_mode_refuses_before_touching_a_device(monkeypatch):
    m = _main()

    def no_device(*a, **k):
        raise AssertionError('a device was asked for')
    monkeypatch.setattr(torch.cuda, 'is_available', no_device)
    base = ['--mode', 'attack', '--restore', 'last']
    for model in ('darknet_d', 'darknet_r', 'darkcapsule', 'darkcapsule2', 'darkcapsule3'):
        with pytest.raises(SystemExit, match='--model capsule, and --model cnn with --cnn_kernels hip'):
            m.main(base + ['--model', model, '--eps', '0,1'])
    with pytest.raises(SystemExit, match='needs --eps'):
        m.main(base + ['--model', 'capsule'])
    for bad in ('0,,1', 'a', '1,-2', '', 'nan', '1;2'):
        with pytest.raises(SystemExit, match='--eps'):
            m.main(base + ['--model', 'capsule', '--eps', bad])
    with pytest.raises(SystemExit, match='Must give restore file'):
        m.main(['--mode', 'attack', '--model', 'capsule', '--eps', '0,1'])
    with pytest.raises(SystemExit, match='--attack_steps'):
        m.main(base + ['--model', 'capsule', '--eps', '1', '--attack', 'pgd', '--attack_steps', '0'])
    a = m.parser.parse_args(base + ['--model', 'capsule', '--eps', '0,1,2,4,8', '--index', '3'])
    assert m.check_attack(a) == [0.0, 1.0, 2.0, 4.0, 8.0] and a.index == 3 and a.index_given
    assert not m.parser.parse_args(base).index_given and m.parser.parse_args(base).index == 0


def test_attack_mode_refuses_the_plain_torch_cnn(tmp_path, monkeypatch):
    import json
    m = _main()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    json.dump(dict(batch_size=8, n_epochs=1, n_classes=43, lr_decay=0.1, dropout=0.0), open(str(tmp_path / 'params.json'), 'w'))
    with pytest.raises(SystemExit, match='cnn_kernels'):
        m.main(['--mode', 'attack', '--model', 'cnn', '--restore', 'last', '--eps', '0,1', '--model_dir', str(tmp_path)])


def test_cabi_declares_and_binds_the_new_entry_points():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name in ('cy_conv_image_grad', 'cy_conv_image_grad_ok', 'cy_attack_step', 'cy_grad_saliency_u8'):
        assert re.search(r'\b%s\s*\(' % name, header)
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6
    assert _lib.query('cy_conv_image_grad_ok', 1024, 32, 32, 256, 9, 0) == 1
    assert _lib.query('cy_conv_image_grad_ok', 2, 32, 32, 64, 4, 1) == 0


def test_package_exports_the_attack_module():
    import capsyolo_amd
    from capsyolo_amd import attack
    assert 'attack' in capsyolo_amd.__all__
    for name in ('input_gradient', 'fgsm', 'pgd', 'robust_accuracy', 'saliency', 'attack_step', 'grad_saliency_u8'):
        assert callable(getattr(attack, name))
    assert attack.GREY == 1 / 128 and (attack.LO, attack.HI) == (-1.0, 127 / 128)
    assert attack.parse_grey_levels('0,1,2.5') == [0.0, 1.0, 2.5]
    with pytest.raises(ValueError):
        attack.parse_grey_levels('1,x')

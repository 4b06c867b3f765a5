"""GPU tests of csrc/image_grad.hip (cy_conv_image_grad) and csrc/attack.hip (cy_attack_step, cy_grad_saliency_u8).

The image gradient is held to the two yardsticks of tests/test_gpu_linear.py: integer inputs, on which every summation order gives
the same fp32 number (exact equality with the int64 result of tests/attack_ref.py), and fp64 on standard-normal inputs, where the
kernel may be 20 x as far from fp64 as torch's CPU fp32 computation of the same gradient is, with a floor of 1e-6.  The shapes are the
smallest that reach each edge: one tile with most taps off the map (12 x 12 under a 9 x 9 kernel), Cout below, at and past a chunk of
8 channels and at the CapsuleNet width, two row tiles (32 rows), a partial row tile and a partial column tile (33 x 32, 7 x 5), k = 1.
The step and saliency kernels are bit-equal to their numpy restatements."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attack_ref
from test_gpu_linear import rel_l2, within_rule

from capsyolo_amd import _lib, ops

pytestmark = pytest.mark.gpu

# (k, pad, H, W, Cout, B)
SHAPES = [(9, 0, 12, 12, c, b) for c in (8, 20, 256) for b in (1, 3)] + \
    [(9, 0, 32, 32, 256, 2), (3, 1, 32, 32, 64, 2), (3, 1, 7, 5, 5, 3), (3, 1, 33, 32, 32, 1), (1, 0, 4, 4, 3, 1)]
LARGEST = [(9, 0, 32, 32, 256, 2), (3, 1, 32, 32, 64, 2)]
GUARD = 64


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def k_image_grad(dy, w, B, H, W, k, pad, act=None, slope=1.0, scale=None):
    """The raw entry point on an output that was NaN and sits between two NaN guard regions, which must stay NaN."""
    n = B * 3 * H * W
    base = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    dx = base[GUARD:GUARD + n].view(B, 3, H, W)
    _lib.call('cy_conv_image_grad', dy.data_ptr(), None if act is None else act.data_ptr(), None if scale is None else scale.data_ptr(),
              w.data_ptr(), dx.data_ptr(), B, H, W, 3, w.shape[0], k, pad, float(slope), _st())
    torch.cuda.synchronize()
    assert torch.isnan(base[:GUARD]).all() and torch.isnan(base[GUARD + n:]).all(), 'the kernel wrote outside dx'
    out = dx.clone()
    assert not torch.isnan(out).any(), 'the kernel left elements of dx unwritten'
    return out


def _variants(with_small_slope):
    """(name, uses act, slope, uses scale): plain; the activation's derivative at slope 0 (and 0.01); the scale; both."""
    v = [('plain', False, 1.0, False), ('act slope 0', True, 0.0, False), ('scale', False, 1.0, True), ('act slope 0 + scale', True, 0.0, True)]
    if with_small_slope:
        v += [('act slope 0.01', True, 0.01, False), ('act slope 0.01 + scale', True, 0.01, True)]
    return v


@functools.lru_cache(maxsize=None)
def int_case(k, pad, H, W, Cout, B):
    """Integers in -2 .. 2 (act too: exact zeros and negatives), scale in powers of two {1, 2, 4}; the int64 results, computed once."""
    rng = np.random.default_rng(100 + k + 3 * H + 5 * W + 7 * Cout + B)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    dy, act = (rng.integers(-2, 3, (B, Ho, Wo, Cout)).astype(np.int64) for _ in range(2))
    w = rng.integers(-2, 3, (Cout, 3, k, k)).astype(np.int64)
    scale = (2 ** rng.integers(0, 3, Cout)).astype(np.int64)
    want, bound = {}, 0
    for name, a, slope, s in _variants(False):
        want[name], mag = attack_ref.image_grad(dy, w, H, W, pad, act if a else None, int(slope), scale if s else None, dtype=np.int64)
        bound = max(bound, int(mag.max()))
    return dict(dy=dy, act=act, w=w, scale=scale, want=want, bound=bound)


@functools.lru_cache(maxsize=None)
def normal_case(k, pad, H, W, Cout, B):
    rng = np.random.default_rng(200 + k + 3 * H + 5 * W + 7 * Cout + B)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    dy, act = (rng.standard_normal((B, Ho, Wo, Cout)).astype(np.float32) for _ in range(2))
    act[rng.random(act.shape) < 0.1] = 0.0                                   # exact zeros: the derivative there is the slope
    w = rng.standard_normal((Cout, 3, k, k)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, Cout).astype(np.float32)
    ref64, cpu32 = {}, {}
    x = torch.zeros(B, 3, H, W, requires_grad=True)
    z = F.conv2d(x, torch.from_numpy(w), None, 1, pad)
    for name, a, slope, s in _variants(True):
        ref64[name], _ = attack_ref.image_grad(dy, w, H, W, pad, act if a else None, slope, scale if s else None)
        dz32 = attack_ref.dz_of(dy, act if a else None, np.float32(slope), scale if s else None).astype(np.float32)
        (g,) = torch.autograd.grad(z, x, torch.from_numpy(np.ascontiguousarray(dz32.transpose(0, 3, 1, 2))), retain_graph=True)
        cpu32[name] = g.numpy().copy()
    return dict(dy=dy, act=act, w=w, scale=scale, ref64=ref64, cpu32=cpu32)


@pytest.mark.parametrize('k,pad,H,W,Cout,B', SHAPES)
def test_exact_on_integers(k, pad, H, W, Cout, B):
    c = int_case(k, pad, H, W, Cout, B)
    assert c['bound'] + 2 < 2 ** 24            # the sum of |terms| of every element: every partial sum of every order is an exact fp32 integer
    assert ops.image_grad_plan((B, 3, H, W), Cout, k, 1, pad).ok
    dy, act, w, scale = _dev(c['dy']), _dev(c['act']), _dev(c['w']), _dev(c['scale'])
    for name, a, slope, s in _variants(False):
        got = k_image_grad(dy, w, B, H, W, k, pad, act if a else None, slope, scale if s else None)
        np.testing.assert_array_equal(got.cpu().numpy(), c['want'][name].astype(np.float32), err_msg=name)
    # the wrapper: same kernel, shape checks in front
    got = ops.conv_image_grad(dy, w, (B, 3, H, W), k, pad, act, 0.0, scale)
    np.testing.assert_array_equal(got.cpu().numpy(), c['want']['act slope 0 + scale'].astype(np.float32))


@pytest.mark.parametrize('k,pad,H,W,Cout,B', SHAPES)
def test_against_fp64(k, pad, H, W, Cout, B):
    c = normal_case(k, pad, H, W, Cout, B)
    dy, act, w, scale = _dev(c['dy']), _dev(c['act']), _dev(c['w']), _dev(c['scale'])
    for name, a, slope, s in _variants(True):
        got = k_image_grad(dy, w, B, H, W, k, pad, act if a else None, slope, scale if s else None)
        within_rule(name, got.cpu().numpy(), c['cpu32'][name], c['ref64'][name])


@pytest.mark.parametrize('k,pad,H,W,Cout,B', LARGEST)
def test_two_runs_identical_bits(k, pad, H, W, Cout, B):
    c = normal_case(k, pad, H, W, Cout, B)
    dy, act, w, scale = _dev(c['dy']), _dev(c['act']), _dev(c['w']), _dev(c['scale'])
    a = k_image_grad(dy, w, B, H, W, k, pad, act, 0.01, scale)
    again = k_image_grad(dy, w, B, H, W, k, pad, act, 0.01, scale)
    assert torch.equal(a.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize('Cin,Cout,k,pad,H,W,slope', [
    (4, 8, 3, 1, 8, 8, 1.0), (3, 8, 4, 1, 8, 8, 1.0), (3, 8, 11, 5, 16, 16, 1.0), (3, 8, 3, 2, 8, 8, 1.0), (3, 1025, 3, 1, 8, 8, 1.0),
    (3, 0, 3, 1, 8, 8, 1.0), (3, 8, 9, 0, 8, 8, 1.0), (3, 8, 3, 1, 8, 8, 1.5), (3, 8, 3, 1, 8, 8, -0.1)])
def test_refused_before_a_launch(Cin, Cout, k, pad, H, W, slope):
    """Every refused shape (and a slope outside [0, 1] beside act) raises, and the output stays as it was."""
    Ho, Wo = max(H + 2 * pad - k + 1, 1), max(W + 2 * pad - k + 1, 1)
    n = max(Cout, 1)
    dy = torch.ones(1, Ho, Wo, n, device='cuda')
    w = torch.ones(n, max(Cin, 1), k, k, device='cuda')
    dx = torch.full((1, max(Cin, 1), H, W), float('nan'), device='cuda')
    with pytest.raises(_lib.HipExtensionError, match='cy_conv_image_grad'):
        _lib.call('cy_conv_image_grad', dy.data_ptr(), dy.data_ptr(), None, w.data_ptr(), dx.data_ptr(), 1, H, W, Cin, Cout, k, pad, slope, _st())
    torch.cuda.synchronize()
    assert torch.isnan(dx).all()
    if slope == 1.0:
        assert _lib.query('cy_conv_image_grad_ok', 1, H, W, Cout, k, pad) == (1 if Cin != 3 else 0)
        assert not ops.image_grad_plan((1, Cin, H, W), Cout, k, 1, pad).ok
        if Cout > 0:                                                              # (the wrapper takes Cout from the weight)
            with pytest.raises(_lib.HipExtensionError, match='conv_image_grad'):
                ops.conv_image_grad(dy, w, (1, Cin, H, W), k, pad)


# ------------------------------------------------------------------------------------------------ the attack step
def _edge_values():
    """4099 elements that contain every edge value: g = 0, -0, NaN, +-inf, denormal-small; x at both eps edges; x0 at lo and hi."""
    rng = np.random.default_rng(11)
    n = 4099
    x0 = ((rng.integers(0, 256, n).astype(np.float32) - 128) / 128).astype(np.float32)
    x = np.clip(x0 + (rng.integers(-2, 3, n) / 128).astype(np.float32), -1, 127 / 128).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    g[:8] = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-38, -1e-38, 3.0]
    x0[8:12] = [-1.0, -1.0, 127 / 128, 127 / 128]
    x[8:12] = x0[8:12]
    g[8:12] = [-1.0, 1.0, 1.0, -1.0]
    x0[12:16] = 0.5
    x[12:16] = [0.5 + 2 / 128, 0.5 + 2 / 128, 0.5 - 2 / 128, 0.5 - 2 / 128]
    g[12:16] = [1.0, -1.0, 1.0, -1.0]
    x[16:20] += np.float32(1e-3)                                                 # off the byte grid: the sums round
    return x, x0, g


@pytest.mark.parametrize('alpha,eps,lo,hi', [(1 / 128, 2 / 128, -1.0, 127 / 128), (0.003, 0.0101, -0.9, 0.9), (0.0, 1 / 128, -1.0, 1.0),
                                             (2 / 128, 0.0, -1.0, 127 / 128)])
def test_attack_step_bit_equal(alpha, eps, lo, hi):
    x, x0, g = _edge_values()
    want = attack_ref.attack_step(x, x0, g, alpha, eps, lo, hi)
    xd, x0d, gd = _dev(x), _dev(x0), _dev(g)
    _lib.call('cy_attack_step', xd.data_ptr(), x0d.data_ptr(), gd.data_ptr(), alpha, eps, lo, hi, xd.numel(), _st())
    got = xd.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(x0d.cpu().numpy().view(np.int32), x0.view(np.int32))     # x0 and g are read only
    with pytest.raises(_lib.HipExtensionError, match='cy_attack_step'):
        _lib.call('cy_attack_step', xd.data_ptr(), x0d.data_ptr(), gd.data_ptr(), -1.0, eps, lo, hi, xd.numel(), _st())


# ------------------------------------------------------------------------------------------------ the saliency map
@pytest.mark.parametrize('B,H,W', [(1, 5, 7), (3, 32, 32)])
def test_saliency_bit_equal(B, H, W):
    rng = np.random.default_rng(5 + B)
    g = (rng.standard_normal((B, 3, H, W)) * 10.0 ** rng.integers(-6, 3, (B, 1, 1, 1))).astype(np.float32)
    if B > 1:
        g[1] = 0.0                                                                # an all-zero image
        g[2, 0, 0, 0], g[2, 1, 3, 3] = np.nan, np.nan
    g[0, 2, 1, 1] = np.nan
    base = torch.zeros(B * H * W + 2 * GUARD, dtype=torch.uint8, device='cuda') + 7
    out = base[GUARD:GUARD + B * H * W].view(B, H, W)
    _lib.call('cy_grad_saliency_u8', _dev(g).data_ptr(), out.data_ptr(), B, H, W, _st())
    want = attack_ref.saliency_u8(g)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert (base[:GUARD] == 7).all() and (base[GUARD + B * H * W:] == 7).all()
    assert want.max() == 255 and (B == 1 or not want[1].any())
    from capsyolo_amd import attack
    np.testing.assert_array_equal(attack.grad_saliency_u8(_dev(g)).cpu().numpy(), want)

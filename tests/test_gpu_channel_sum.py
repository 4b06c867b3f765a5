"""GPU tests of cy_channel_sum_ws (csrc/conv.hip): the bias gradient of a convolution without BatchNorm, out[n] = sum over the rows of
dZ [P, N], with cy_channel_sum's row splits but added in a fixed order through a workspace of partials.  Two runs on the same non-integer
input give the same bits (cy_channel_sum, which adds its splits with float atomics, does not promise that); the values are held to
float64 with a bound that follows from the order of the sum; the sizes sit at the edges of the split rule:
    splits = min(ceil(2048 / ceil(N / 64)), ceil(P / 64)), rows per split = ceil(P / splits)
P = 64 | 65 (one split | two), P = 2048 * 64 and one more row (the cap of 2048 splits for up to 64 channels), N = 64 | 65 (one | two
channel blocks), N = 3 and 70 (part of a block), and CapsuleNet's own layers at batch 32 (conv1: 18432 x 256, decoder: 32768 x 16).

Measured on the MI355X: largest error / bound 0.030 (P = 64), 0.014 and 0.007 on CapsuleNet's two layers; equal bits in every repeat."""
import ctypes as C

import numpy as np
import pytest
import torch

from capsyolo_amd import _lib, ops

pytestmark = pytest.mark.gpu

SHAPES = [(64, 16), (65, 16), (65, 3), (1000, 70), (5000, 64), (5000, 65), (18432, 256), (32768, 16), (2048 * 64, 3), (2048 * 64 + 1, 3),
          (2048 * 64 + 1, 64)]


def _split_rule(P, N):
    nb = (N + 63) // 64
    sp = min(-(-2048 // nb), -(-P // 64))
    rpb = -(-P // sp)
    return -(-P // rpb), rpb


def _input(P, N):
    g = torch.Generator().manual_seed(1000 * N + P % 997)
    return (torch.randn((P, N), generator=g) * (1.0 + torch.arange(N, dtype=torch.float32) / N) + 0.25).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run_ws(dz, ws_fill):
    P, N = dz.shape
    need = _lib.query('cy_channel_sum_ws_floats', P, N)
    out = torch.full((N,), float('nan'), device='cuda')
    ws = torch.full((max(need, N),), ws_fill, device='cuda')            # (one split still writes its N sums) not initialised: two different fills
    _lib.call('cy_channel_sum_ws', C.c_void_p(dz.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), P, N, _stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('P,N', SHAPES)
def test_fixed_order_sum(P, N):
    """Equal bits in three runs (the workspace filled with NaN, with 1e30 and with NaN again beforehand), and against float64 within
    depth * 2^-24 * sum |dz| per channel, depth = the longest chain of fp32 additions any element passes through: ceil(rows per
    split / 4) in its wave's running sum, 3 across the four waves, ceil(splits / 16) in the finish kernel's running sum, 4 in its tree."""
    splits, rpb = _split_rule(P, N)
    need = _lib.query('cy_channel_sum_ws_floats', P, N)
    assert need == (splits * N if splits > 1 else 0)
    dz = _input(P, N)
    runs = [_run_ws(dz, fill) for fill in (float('nan'), 1e30, float('nan'))]
    assert all(torch.equal(runs[0].view(torch.int32), r.view(torch.int32)) for r in runs[1:])
    want = dz.double().sum(0)
    depth = -(-rpb // 4) + 3 + -(-splits // 16) + 4
    bound = depth * 2.0 ** -24 * dz.double().abs().sum(0)
    frac = float(((runs[0].double() - want).abs() / bound).max())
    print('P %d N %d: %d splits of %d rows, largest error / bound %.3g' % (P, N, splits, rpb, frac))
    assert torch.isfinite(runs[0]).all() and frac <= 1.0


def test_edges_of_the_split_rule():
    assert _lib.query('cy_channel_sum_ws_floats', 64, 16) == 0 and _lib.query('cy_channel_sum_ws_floats', 65, 16) == 2 * 16
    # at the cap of 2048 splits one more row makes the splits 65 rows long, and 2017 of them cover it
    assert _lib.query('cy_channel_sum_ws_floats', 2048 * 64, 3) == 2048 * 3 and _lib.query('cy_channel_sum_ws_floats', 2048 * 64 + 1, 3) == 2017 * 3
    assert all(_lib.query('cy_channel_sum_ws_floats', P, N) == (_split_rule(P, N)[0] * N if _split_rule(P, N)[0] > 1 else 0) for P, N in SHAPES)
    assert _lib.query('cy_channel_sum_ws_floats', 10 ** 6, 65) == 1024 * 65
    assert _lib.query('cy_channel_sum_ws_floats', 0, 8) == 0


def test_a_small_workspace_is_refused():
    dz = _input(5000, 64)
    need = _lib.query('cy_channel_sum_ws_floats', 5000, 64)
    out, ws = torch.zeros(64, device='cuda'), torch.zeros(need - 1, device='cuda')
    with pytest.raises(_lib.HipExtensionError, match='workspace holds'):
        _lib.call('cy_channel_sum_ws', C.c_void_p(dz.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, 5000, 64, _stream())
    assert not out.cpu().numpy().any()


@pytest.mark.parametrize('P,N', [(50, 8), (64, 16), (5000, 64), (32768, 16)])
def test_ops_channel_sum_repeats_and_matches_the_atomic_sum(P, N):
    """ops.channel_sum (what the backward of a convolution without BatchNorm calls) takes cy_channel_sum for one split and cy_channel_sum_ws
    for more, gives equal bits twice, and agrees with cy_channel_sum (the split sum with atomics: the same partial sums, added in
    another order) within splits * 2^-24 * sum |dz|."""
    dz = _input(P, N)
    _lib.TRACE = trace = []
    try:
        a, b = ops.channel_sum(dz, N), ops.channel_sum(dz, N)
    finally:
        _lib.TRACE = None
    splits, _ = _split_rule(P, N)
    assert trace == ['cy_channel_sum' if splits == 1 else 'cy_channel_sum_ws'] * 2
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    old = torch.empty(N, device='cuda')
    _lib.call('cy_channel_sum', C.c_void_p(dz.data_ptr()), C.c_void_p(old.data_ptr()), P, N, _stream())
    assert float(((a.double() - old.double()).abs() / ((splits + 1) * 2.0 ** -24 * dz.double().abs().sum(0))).max()) <= 1.0
    if splits == 1:
        assert torch.equal(a.view(torch.int32), old.view(torch.int32))


def test_bias_gradient_of_a_convolution_repeats():
    """The backward of a HipConv2d without BatchNorm (16 -> 8 channels, 3 x 3, batch 4, 24 x 24: 2304 rows, 36 splits) twice on the
    same input: the bias gradient has the same bits, and equals the float64 sum of the output gradient within the bound above."""
    from capsyolo_amd import models
    torch.manual_seed(4)
    conv = models.HipConv2d(16, 8, 3, 1, 1).cuda()
    x = torch.randn(4, 24, 24, 16, device='cuda')
    g = torch.randn(4, 24, 24, 8, device='cuda')
    grads = []
    for _ in range(2):
        conv.zero_grad()
        y = conv(x)
        assert y.shape == g.shape
        y.backward(g)
        grads.append(conv.bias.grad.clone())
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    want = g.double().sum((0, 1, 2))
    np.testing.assert_allclose(grads[0].double().cpu().numpy(), want.cpu().numpy(), rtol=0, atol=float(32 * 2.0 ** -24 * g.double().abs().sum((0, 1, 2)).max()))

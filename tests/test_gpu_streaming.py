"""GPU tests of csrc/bn.hip, csrc/misc.hip and cy_channel_sum on the case table of tests/stream_cases.py (validated on the CPU by
tests/test_stream_cases_host.py): every kernel against a float64 reference written from the definition, at the shapes where its
launcher takes another path.  Every output starts as NaN, so an element that a kernel leaves unwritten shows; the deterministic
kernels run twice for equal bits: all but cy_channel_sum on non-integer input (float atomics) and cy_bn_bwd_reduce with more than two
row blocks (double atomics between the blocks), whose two runs are held to the rounding of a double sum.  Tolerances: see stream_cases."""
import numpy as np
import pytest
import torch

import stream_cases as S
from capsyolo_amd._lib import HipExtensionError, call

pytestmark = pytest.mark.gpu


def _check(name):
    c = S.case(name)
    K = S.Kernels()
    got = S.run(c, K)
    fr = S.fractions(c, got)
    for k, v in sorted(fr.items()):
        print('RATIO %s %s %.3g' % (name, k, v))
    S.compare(c, got)
    for k, v in got.items():
        assert v.dtype == (np.int64 if k == 'nbt' else np.float64 if k in ('red', 'red_out') else np.float32), (k, v.dtype)
    if c['kind'] == 'channel_sum' and not c['exact']:
        return got
    again = S.run(c, K)
    if c['kind'] == 'bn_bwd_reduce':
        # the row blocks of cy_bn_bwd_reduce add their double partial sums to red with atomics: up to two blocks a channel the order
        # cannot matter (a + b = b + a), behind that two runs may differ by the rounding of a double sum of nb partials in another
        # order, 2 (nb - 1) 2^-53 of the terms' abs-sum at the most (measured at nb = 1844: differing bits)
        rpar, rpb, _ = S.reduce_plan(c['P'], c['N'])
        nb = S.ceil_div(c['P'], rpb)
        if nb > 2:
            bound = 2.0 * (nb - 1) * 2.0 ** -53 * S.reference(name)['mag:red']
            diff = np.abs(got['red'] - again['red'])
            print('REPEAT %s: %d row blocks, largest difference / bound %.3g' % (name, nb, float((diff / bound).max())))
            assert (diff <= bound).all()
            return got
    for k, v in got.items():
        assert v.tobytes() == again[k].tobytes(), '%s: %s differs between two runs' % (name, k)
    return got


@pytest.mark.parametrize('name', S.names(big=False))
def test_case(name):
    _check(name)


@pytest.mark.parametrize('name', sorted(S.BIG))
def test_large_case(name):
    _check(name)
    S._refs.clear()
    torch.cuda.empty_cache()


def test_softmax_over_one_class_is_exactly_one_with_a_gradient_of_exactly_zero():
    got = S.run(S.case('yolo_head/one_class'), S.Kernels())
    assert (got['y'][:, -1] == 1).all() and not got['dx'][:, -1].any()


@pytest.mark.parametrize('N', S.REFUSED_REDUCE_N)
def test_reduce_refuses_a_channel_count_it_has_no_layout_for(N):
    P = 8
    t = [torch.ones(P, N, device='cuda') for _ in range(2)] + [torch.ones(N, device='cuda') for _ in range(4)]
    red = torch.zeros(N, 2, dtype=torch.float64, device='cuda')
    with pytest.raises(HipExtensionError, match='cy_bn_bwd_reduce'):
        call('cy_bn_bwd_reduce', *[v.data_ptr() for v in t], 0.1, red.data_ptr(), P, N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not red.any()


# ------------------------------------------------------------------------------------------------ above the grid cap
def _device_inputs(kind, seed):
    """z (and the gradient) of an ABOVE_CAP case, drawn on the device; every argument z scale + shift at least MARGIN from 0 in float64."""
    a = S.ABOVE_CAP[kind]
    P, N = a['P'], a['N']
    scale, shift = S._scale_shift(np.random.default_rng(seed), N)
    sc, sh = torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda()          # float64
    gen = torch.Generator(device='cuda').manual_seed(seed)
    z = torch.empty(P, N, device='cuda')
    step = 1 << 16
    for r in range(0, P, step):                                          # in row chunks: no float64 copy of the whole tensor
        zc = z[r:r + step]
        zc.normal_(generator=gen)
        y = zc.double() * sc + sh
        target = torch.where(y < 0, -4 * S.MARGIN, 4 * S.MARGIN)
        zc.copy_(torch.where(y.abs() < S.MARGIN, (target - sh) / sc, zc.double()).float())
        assert float((zc.double() * sc + sh).abs().min()) >= S.MARGIN
    return P, N, z, sc, sh, gen


def _slabs(n, straddle):
    """Three slabs of 2^20 elements of a flat tensor of n: the first, the last, one around `straddle`."""
    m = 1 << 20
    return [(0, m), (n - m, n), (straddle - m // 2, straddle + m // 2)]


def _rule(name, got, ref, mag, ref32):
    """The tolerance rule of stream_cases on one slab (torch float64 on the device; ref32: the float32 CPU evaluation)."""
    e = float(((got.double() - ref).abs() / mag).max())
    e32 = float(((ref32.double().cuda() - ref).abs() / mag).max())
    tol = max(1e-6, 20.0 * e32)
    print('RATIO %s %.3g' % (name, e / tol))
    assert np.isfinite(e) and e <= tol, (name, e, tol)


def test_affine_act_above_the_grid_cap():
    """9 x 65536 x 256 float4 and a remainder: a thread of the 65536-block grid runs the unrolled body twice, then the tail."""
    P, N, z, sc, sh, _ = _device_inputs('affine_act', 71)
    slope = 0.1
    a = torch.full_like(z, float('nan'))
    scf, shf = sc.float(), sh.float()
    call('cy_affine_act', z.data_ptr(), a.data_ptr(), scf.data_ptr(), shf.data_ptr(), slope, P, N, torch.cuda.current_stream().cuda_stream)
    stride = S.STREAM_CAP * 256 * 4                                      # the grid stride in elements
    for lo, hi in _slabs(P * N, 8 * stride):
        assert lo % N == 0
        zs, got = z.view(-1)[lo:hi].view(-1, N), a.view(-1)[lo:hi].view(-1, N)
        y = zs.double() * sc + sh
        ref = torch.where(y > 0, y, y * slope)
        mag = ((zs.double() * sc).abs() + sh.abs()) * torch.where(y > 0, 1.0, slope)
        y32 = zs.cpu() * scf.cpu() + shf.cpu()
        _rule('affine_act/above_cap[%d:%d]' % (lo, hi), got, ref, mag, torch.where(y32 > 0, y32, y32 * np.float32(slope)))
    del z, a
    torch.cuda.empty_cache()


def test_bn_bwd_apply_above_the_grid_cap():
    """5 x 65536 x 256 float4 and a remainder: the unrolled body (two float4 a pass) twice, then the tail."""
    P, N, z, sc, sh, gen = _device_inputs('bn_bwd_apply', 72)
    slope = 0.1
    rng = np.random.default_rng(73)
    mean, invstd = (torch.from_numpy(v).cuda() for v in S._mean_invstd(rng, N))
    red = torch.from_numpy(rng.standard_normal((N, 2)) * np.sqrt(P) * 3.0).cuda()
    da = torch.empty_like(z).normal_(generator=gen)
    dz = torch.full_like(z, float('nan'))
    f = [v.float() for v in (sc, sh, mean, invstd)]
    dgamma, dbeta = torch.full((N,), float('nan'), device='cuda'), torch.full((N,), float('nan'), device='cuda')
    call('cy_bn_bwd_apply', z.data_ptr(), da.data_ptr(), dz.data_ptr(), *[v.data_ptr() for v in f], None, slope, red.data_ptr(), dgamma.data_ptr(),
         dbeta.data_ptr(), P, N, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(dbeta, red[:, 0].float()) and torch.equal(dgamma, red[:, 1].float())
    stride = S.STREAM_CAP * 256 * 4
    means = red * (1.0 / P)
    m32 = means.float().cpu()
    for lo, hi in _slabs(P * N, 4 * stride):
        assert lo % N == 0
        zs, gs, got = (t.view(-1)[lo:hi].view(-1, N) for t in (z, da, dz))
        y = zs.double() * sc + sh
        d = torch.where(y > 0, gs.double(), gs.double() * slope)
        xh = (zs.double() - mean) * invstd
        m1, m2 = means[:, 0], means[:, 1]
        ref = sc * (d - m1 - xh * m2)
        mag = sc.abs() * (d.abs() + m1.abs() + (xh * m2).abs())
        zc, gc = zs.cpu(), gs.cpu()
        c32 = [v.cpu() for v in f]
        y32 = zc * c32[0] + c32[1]
        d32 = torch.where(y32 > 0, gc, gc * np.float32(slope))
        _rule('bn_bwd_apply/above_cap[%d:%d]' % (lo, hi), got, ref, mag, c32[0] * (d32 - m32[:, 0] - (zc - c32[2]) * c32[3] * m32[:, 1]))
    del z, da, dz
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the block that pools an odd map
@pytest.mark.parametrize('train', [True, False])
def test_backbone_pools_an_odd_map(train):
    """conv-bn-lrelu-maxpool twice on a 20 x 20 input: maps 10 -> 5 -> 2.  The second pooling has an odd map, which the fused
    activation + pooling pass does not take (ops.pool_fusable): it runs ops.maxpool2, which must floor like nn.MaxPool2d(2).
    Against the same torch modules in float64 at the tolerances of test_conv_bn_lrelu_block."""
    from capsyolo_amd import models
    from test_gpu_kernels import close, rnd
    torch.manual_seed(5)
    cin, c1, c2, B = 32, 64, 64, 3
    convs = [torch.nn.Conv2d(cin, c1, 4, 2, 1).double(), torch.nn.Conv2d(c1, c2, 3, 1, 1).double()]
    bns = [torch.nn.BatchNorm2d(c1).double(), torch.nn.BatchNorm2d(c2).double()]
    for bn in bns:
        n = bn.num_features
        bn.weight.data = 1 + 0.2 * torch.randn(n).double()
        bn.bias.data = 0.1 * torch.randn(n).double()
        bn.running_mean.data = 0.1 * torch.randn(n).double()
        bn.running_var.data = 1 + 0.2 * torch.rand(n).double()
    ref = torch.nn.Sequential(convs[0], bns[0], torch.nn.LeakyReLU(0.1), torch.nn.MaxPool2d(2),
                              convs[1], bns[1], torch.nn.LeakyReLU(0.1), torch.nn.MaxPool2d(2)).train(train)
    seq = models.FusedBackbone()
    for i, (conv, bn, geo) in enumerate(zip(convs, bns, [(cin, c1, 4, 2, 1), (c1, c2, 3, 1, 1)]), 1):
        seq.add_module('conv_%d' % i, models.HipConv2d(*geo))
        seq.add_module('bn_%d' % i, models.HipBatchNorm2d(geo[1]))
        seq.add_module('relu_%d' % i, models.HipLeakyReLU(0.1))
        seq.add_module('maxpool_%d' % i, models.HipMaxPool2())
        getattr(seq, 'conv_%d' % i).load_state_dict({k: v.float() for k, v in conv.state_dict().items()})
        getattr(seq, 'bn_%d' % i).load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in bn.state_dict().items()})
    seq.to('cuda').train(train)
    x = rnd((B, cin, 20, 20), 8)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    assert tuple(yr.shape) == (B, c2, 2, 2)
    xh = x.permute(0, 2, 3, 1).contiguous().to('cuda').requires_grad_(True)
    yh = seq(xh, nchw_in=False)
    close(yh.permute(0, 3, 1, 2), yr, 1e-4, 1e-5)
    for i, bn in enumerate(bns, 1):
        close(getattr(seq, 'bn_%d' % i).running_mean, bn.running_mean, 1e-4, 1e-6)
        close(getattr(seq, 'bn_%d' % i).running_var, bn.running_var, 1e-4, 1e-6)
    if train:
        g = rnd(tuple(yr.shape), 9)
        yr.backward(g.double())
        yh.backward(g.permute(0, 2, 3, 1).contiguous().to('cuda'))
        close(xh.grad.permute(0, 3, 1, 2), xr.grad, 1e-3, 1e-4)
        for i, (conv, bn) in enumerate(zip(convs, bns), 1):
            close(getattr(seq, 'conv_%d' % i).weight.grad, conv.weight.grad, 1e-3, 1e-4)
            close(getattr(seq, 'bn_%d' % i).weight.grad, bn.weight.grad, 1e-3, 1e-4)
            close(getattr(seq, 'bn_%d' % i).bias.grad, bn.bias.grad, 1e-3, 1e-4)


# ------------------------------------------------------------------------------------------------ the statistics of the conv epilogues
@pytest.mark.parametrize('k,fwd,adds', [(1, 'conv_gemm_fwd', 33), (3, 'conv_wino_fwd', 65)])
def test_conv_statistics_on_channels_with_a_large_mean(k, fwd, adds):
    """The conv epilogues add v and v v in float32 per lane before the double atomics (csrc/conv.hip: 32 values a lane and one
    cross-lane add, 33 additions; csrc/winograd.hip: 64 values and one, 65), and cy_bn_finalize forms s2 / count - m^2.  Channels with
    |mean| / std of about 0, 10 and 100 (a bias on constant-plus-noise input): invstd against the float64 statistics of the z the
    kernel itself wrote.  Only the derivable bound is asserted: (adds + 2) 2^-24 (1 + m^2 / var), relative.  Measured: DESIGN.md 6o."""
    from capsyolo_amd import ops
    B, H, W, Cin, Cout, eps = 4, 16, 16, 32, 96, 1e-5
    gen = torch.Generator().manual_seed(91 + k)
    x = 1.0 + 0.1 * torch.randn(B, Cin, H, W, generator=gen)
    w = 0.1 * torch.randn(Cout, Cin, k, k, generator=gen)
    z0 = torch.nn.functional.conv2d(x.double(), w.double(), None, padding=k // 2)
    ratio = torch.tensor([0.0, 10.0, 100.0]).repeat(Cout // 3)
    bias = (ratio * z0.std(dim=(0, 2, 3), unbiased=False) - z0.mean(dim=(0, 2, 3))).float()
    assert ops.conv_plan((B, H, W, Cin), Cout, k, 1, k // 2).fwd == fwd
    xg = x.permute(0, 2, 3, 1).contiguous().cuda()
    stats = torch.zeros((ops.STATS_COPIES, Cout, 2), dtype=torch.float64, device='cuda')
    z = ops.conv_forward(xg, w.cuda(), bias.cuda(), k, 1, k // 2, False, stats, False)
    P = B * H * W
    ones, zeros = torch.ones(Cout, device='cuda'), torch.zeros(Cout, device='cuda')
    o = [torch.full((Cout,), float('nan'), device='cuda') for _ in range(4)]
    call('cy_bn_finalize', stats.data_ptr(), P, ones.data_ptr(), zeros.data_ptr(), None, None, 0.1, eps, *[v.data_ptr() for v in o], Cout, None,
         torch.cuda.current_stream().cuda_stream)
    zz = z.double().reshape(P, Cout)
    m, var = zz.mean(0), zz.var(0, unbiased=False)
    want = 1.0 / torch.sqrt(var + eps)
    rel = ((o[3].double() - want).abs() / want).cpu()
    bound = ((adds + 2) * 2.0 ** -24 * (1.0 + m * m / var)).cpu()
    for i, r in enumerate((0, 10, 100)):
        got_ratio = float((m.abs() / var.sqrt()).cpu()[i::3].mean())
        print('STATS k=%d |mean|/std %.1f: largest relative error of invstd %.3g, bound %.3g, error / bound %.3g'
              % (k, got_ratio, float(rel[i::3].max()), float(bound[i::3].min()), float((rel / bound)[i::3].max())))
        assert abs(got_ratio - r) < 0.05 * r + 0.3
    assert bool((rel <= bound).all())

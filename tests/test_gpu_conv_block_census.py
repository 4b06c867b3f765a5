"""The launch sequence of the conv blocks (ops.conv_block / ops.conv_block_bf16 / ops.affine_act_maxpool under FusedBackbone) is
locked: tests/golden/conv_block_census.json holds, for every case of tests/conv_block_cases.py, the ordered C-ABI entry points of
one training forward + backward (and one eval forward).  The file was recorded BEFORE the blocks were split into one Function per
kind and the hand-over between blocks became ops.BnHandover, its bf16_unfused / bf16_odd / bf16_apply_only cases BEFORE the bf16
path's decisions moved into ops.conv_plan_bf16; it is not regenerated to make this test pass."""
import json
import os

import numpy as np
import pytest
import torch

import conv_block_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_block_census.json')


def close(a, b, rtol, atol_rel):
    """test_gpu_kernels.close: the absolute part is relative to the largest reference value."""
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_rel * np.abs(b).max())


def test_the_table_and_the_recorded_file_cover_the_same_cases():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(cases.CASES)
    flat = dict((name, [n for phase in sorted(c) for n in c[phase]]) for name, c in golden.items())
    # the recorded lists reach the branch each case is there for
    assert [n for n, calls in sorted(flat.items()) if 'cy_conv1_bn_bwd_onepass_mask' in calls] == ['c1_mask']
    assert 'cy_conv1_bn_bwd_onepass' in flat['c1_onepass'] and 'cy_conv1_bn_bwd_wgrad' in flat['c1_twopass']
    assert 'cy_conv1_bn_bwd_reduce' not in flat['c1_defer'] and flat['c1_defer'].count('cy_bn_bwd_reduce') == 1
    assert 'cy_conv3x3_winograd_wgrad_bn' in flat['defer_s2'] and flat['defer_s2'].count('cy_bn_bwd_reduce') == 1
    assert 'cy_maxpool2_bwd_bn' in flat['pool'] and 'cy_bn_bwd_reduce' not in flat['pool']
    assert 'cy_conv_wgrad_bf16_bn' in flat['bf16'] and 'cy_conv1_bn_bwd_reduce_bf16' in flat['bf16']
    assert 'cy_act_bwd' in golden['nobn']['train_slope_0.1'] and 'cy_act_bwd' not in golden['nobn']['train_slope_None']
    # bf16_unfused: two forwards, block 3's input gradient class by class (four), block 2's one class -- and every block sums and
    # applies for itself
    assert flat['bf16_unfused'].count('cy_conv_gemm_bf16') == 7 and 'cy_conv_gemm_bf16_classes' not in flat['bf16_unfused']
    assert 'cy_conv_wgrad_bf16_bn' not in flat['bf16_unfused'] and flat['bf16_unfused'].count('cy_bn_bwd_apply_bf16') == 2
    assert 'cy_conv_wgrad_bf16_bn' not in flat['bf16_apply_only'] and 'cy_conv_gemm_bf16_classes' in flat['bf16_apply_only']
    # bf16_odd: block 3's input gradient (between its weight gradient and the fold of the sums it took for block 2) is four launches
    odd = flat['bf16_odd']
    dgrad3 = odd[odd.index('cy_conv_wgrad_bf16') + 1:odd.index('cy_bn_red_fold')]
    assert 'cy_conv_gemm_bf16_classes' not in odd and dgrad3.count('cy_conv_gemm_bf16') == 4 and 'cy_conv_wgrad_bf16_bn' in odd


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_conv_block_launch_census(name, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = cases.census(name, monkeypatch.setattr)
    assert sorted(got) == sorted(want)
    for phase in sorted(want):
        assert got[phase] == want[phase], (name, phase)


def test_two_steps_with_the_same_cfg_objects():
    """defer_s2 driven block by block with ONE pair of ConvBlockCfg objects for two forward + backward steps: no forward or
    backward writes to a cfg (the hand-over travels with the output), and the second step's parameter gradients are those of
    the first (the statistics are sums of double atomics, so to tolerance, not to the bit)."""
    from capsyolo_amd import ops
    case = cases.CASES['defer_s2']
    net = cases.build_net(case, torch.device('cuda:0'))
    x = cases.case_input(case, torch.device('cuda:0'))
    (c1, b1), (c2, b2) = (net.conv_1, net.bn_1), (net.conv_2, net.bn_2)
    cfg1 = ops.ConvBlockCfg(c1.k, c1.stride, c1.padding, False, b1, 0.1, 'conv_1', defer_act=True)
    cfg2 = ops.ConvBlockCfg(c2.k, c2.stride, c2.padding, False, b2, 0.1, 'conv_2')
    before = [dict(vars(c)) for c in (cfg1, cfg2)]
    grads = []
    for _ in range(2):
        ops.zero_pool.reset(x.device)
        net.zero_grad(set_to_none=True)
        x.grad = None
        z, h = ops.conv_block(x, c1.weight, c1.bias, b1.weight, b1.bias, cfg1)
        assert isinstance(h, ops.BnHandover)
        y = ops.conv_block(z, c2.weight, c2.bias, b2.weight, b2.bias, cfg2, h)
        y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        assert h.take_red() is None                          # the producer's backward took what the consumer gave
        grads.append([(n, p.grad.clone()) for n, p in net.named_parameters()] + [('x', x.grad.clone())])
    assert [dict(vars(c)) for c in (cfg1, cfg2)] == before
    assert len(grads[0]) == 9
    for (n, a), (_, b) in zip(grads[1], grads[0]):
        close(a, b, 1e-3, 1e-4)

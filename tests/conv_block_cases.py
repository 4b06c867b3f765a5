"""The block cases of the conv-block launch census: one small table, shared by tests/golden/make_golden_conv_block_census.py
(which records) and tests/test_gpu_conv_block_census.py (which compares).  A case is a FusedBackbone of conv -> BatchNorm ->
LeakyReLU (-> MaxPool2) blocks, or a bare HipConv2d, at the smallest shape that still reaches its branch of ops.conv_block /
ops.conv_block_bf16; what is recorded is the ORDERED list of C-ABI entry points (_lib.TRACE) of one training forward + backward
and, where `eval` is set, of one eval forward under torch.no_grad()."""
import torch

C1 = [(3, 32, 3, 1, 1)]
BF16 = [(3, 64, 3, 1, 1), (64, 128, 3, 1, 1), (128, 128, 4, 2, 1)]     # fp32 first block, then two blocks on the bf16 kernels
# name -> blocks (cin, cout, k, stride, pad), input shape, layout, and what the case switches
CASES = {
    'c1_mask': dict(blocks=C1, x=(2, 3, 8, 32), nchw=True, switches={'CONV1_MOMENTS_MIN_PIXELS': 0}),
    'c1_onepass': dict(blocks=C1, x=(2, 3, 8, 32), nchw=True, switches={'CONV1_MOMENTS_MIN_PIXELS': 0, 'CONV1_SIGNMASK': False}),
    'c1_twopass': dict(blocks=C1, x=(2, 3, 8, 32), nchw=True, switches={'CONV1_MOMENTS_MIN_PIXELS': 1 << 62}, eval=True),
    'c1_defer': dict(blocks=[(3, 64, 3, 1, 1), (64, 64, 4, 2, 1)], x=(2, 3, 8, 32), nchw=True),
    'defer_s2': dict(blocks=[(64, 64, 3, 1, 1), (64, 64, 4, 2, 1)], x=(2, 12, 12, 64), nchw=False, x_grad=True, eval=True),
    'pool': dict(blocks=[(16, 32, 3, 1, 1)], x=(2, 8, 8, 16), nchw=False, pool=True),
    'nobn': dict(conv=(16, 8, 3, 1, 1), slopes=(None, 0.0, 0.1), x=(2, 5, 5, 16), nchw=False),
    'bf16': dict(blocks=BF16, x=(2, 3, 8, 32), nchw=True, precision='bf16', eval=True),
    # every block sums for itself and applies with cy_bn_bwd_apply_bf16; block 3's input gradient is one launch per parity class
    'bf16_unfused': dict(blocks=BF16, x=(2, 3, 8, 32), nchw=True, precision='bf16',
                         switches={'FUSE_BN_BWD_APPLY_BF16': False, 'FUSE_BN_BWD_REDUCE_BF16': False, 'BF16_DGRAD_ONE_LAUNCH': False}),
    # block 3 reads a 9 x 32 map: its parity classes differ in size, so they go out one by one although the switch is on
    'bf16_odd': dict(blocks=BF16, x=(2, 3, 9, 32), nchw=True, precision='bf16'),
    # no gradient arrives premasked, so no block takes cy_conv_wgrad_bf16_bn although its switch is on
    'bf16_apply_only': dict(blocks=BF16, x=(2, 3, 8, 32), nchw=True, precision='bf16', switches={'FUSE_BN_BWD_REDUCE_BF16': False}),
}


def build_net(case, device):
    """The case's FusedBackbone (training mode) with torch's default initialisation under a fixed seed."""
    from capsyolo_amd import models
    torch.manual_seed(3)
    seq = models.FusedBackbone()
    for i, (cin, cout, k, s, p) in enumerate(case['blocks'], 1):
        seq.add_module('conv_%d' % i, models.HipConv2d(cin, cout, k, s, p))
        seq.add_module('bn_%d' % i, models.HipBatchNorm2d(cout))
        seq.add_module('relu_%d' % i, models.HipLeakyReLU(0.1))
    if case.get('pool'):
        seq.add_module('maxpool_1', models.HipMaxPool2())
    if 'precision' in case:
        seq.precision = case['precision']
    return seq.to(device).train()


def case_input(case, device, seed=17):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case['x'], generator=g).to(device)
    return x.requires_grad_() if case.get('x_grad') else x


def _traced(fn):
    from capsyolo_amd import _lib
    _lib.TRACE = []
    try:
        fn()
        torch.cuda.synchronize()
        return list(_lib.TRACE)
    finally:
        _lib.TRACE = None


def _step(net, x, **kw):
    y = net(x, **kw)
    y.backward(torch.ones_like(y))


def census(name, setattr_):
    """{phase: [entry-point names in call order]} of one case.  setattr_(obj, attr, value) sets an ops switch and is the
    caller's to undo (pytest's monkeypatch.setattr, or the generator's own)."""
    from capsyolo_amd import models, ops
    case, device = CASES[name], torch.device('cuda:0')
    for k, v in case.get('switches', {}).items():
        setattr_(ops, k, v)
    x = case_input(case, device)
    # whatever ran before in this process, the zero pool is in ONE state: it exists and has been used since its last reset,
    # so every training forward of a FusedBackbone starts with cy_zero_bytes
    ops.zero_pool.reset(device)
    ops.zero_pool.take((1,), torch.float64, device)
    if 'conv' in case:
        torch.manual_seed(3)
        conv = models.HipConv2d(*case['conv']).to(device)
        return dict(('train_slope_%s' % s, _traced(lambda: _step(conv, x, nchw_in=case['nchw'], slope=s))) for s in case['slopes'])
    net = build_net(case, device)
    out = {'train': _traced(lambda: _step(net, x, nchw_in=case['nchw']))}
    if case.get('eval'):
        net.eval()
        with torch.no_grad():
            out['eval'] = _traced(lambda: net(x, nchw_in=case['nchw']))
    return out

"""The first block's sign mask (csrc/conv1.hip): the activation pass of the forward stores one bit per element, y > 0, and the
one-pass backward reads that bit instead of recomputing z (cy_conv1_3x3_fwd_act_mask / cy_conv1_bn_bwd_onepass_mask).

What is held here:
  * the forward's activation bytes are those of cy_conv1_3x3_fwd, with and without a mask;
  * the mask's content and LAYOUT: bit (r, nt) of lane (li, lh) of a tile == y > 0, packed on the host (a packing with r and nt
    swapped is a different answer, and one flipped bit moves exactly its channel's sum of d).  y is the backward's
    y = fma(conv + bias, scale, shift); its sign is taken here from the layer's own z in double (a product of two floats and a sum
    with a third keep their sign in double).  Without a bias that is the y of the stored activation, and the bit must equal
    stored activation > 0 everywhere; with a bias the activation comes from fma(conv, scale, bias * scale + shift), which may round
    to the other side of zero, so there the test counts such elements, prints the count and compares the bit with stored
    activation > 0 on all the others;
  * the backward is cy_conv1_bn_bwd_onepass to the bit (torch.equal on dW, dgamma, dbeta, the striped sums of d and red_out), with and
    without a bias: the tile walk, the MFMA order of dW and the order of every sum are unchanged, and the bit is what the recompute
    path computes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOPE = 0.1
COPIES = 16           # CY_STATS_COPIES


def dev():
    return torch.device('cuda:0')


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def walk_shape():
    """A shape on which a persistent wave walks more than one tile: conv1_blocks() launches min(ceil(tiles / 4), CUs) blocks of 4
    waves, so tiles must exceed 4 * CUs -- and not by a multiple, so that some waves walk two tiles and the others one."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, W = 3, 64
    H = (4 * cus) // (B * (W // 32)) + 11
    tiles = B * H * (W // 32)
    assert 4 * cus < tiles < 8 * cus and tiles % (4 * cus) != 0
    return B, H, W


SHAPES = [(1, 1, 32), (2, 3, 32), (3, 5, 96), 'walk']


def pack_expected(act, nt_tiles, swap=False):
    """The sign words as the header describes them, from the stored activation [B][H][W][Cout] (numpy): per 32-pixel tile and
    lane (li = lane % 32, lh = lane / 32) the elements e = NT r + nt -- pixel (r & 3) + 8 (r >> 2) + 4 lh, channel NT li + nt --
    fill words of n = min(32, 16 NT) bits from the top bit down.  swap: the (wrong) order e = 16 nt + r."""
    NT = nt_tiles
    cout = 32 * NT
    a = (act.reshape(-1, 32, 32, NT) > 0)                       # [tile][pixel][li][nt]
    r = np.arange(16)
    p = ((r & 3) + 8 * (r >> 2))[None, :] + 4 * np.arange(2)[:, None]      # [lh][r]
    b = a[:, p]                                                 # [tile][lh][r][li][nt]
    b = b.transpose(0, 1, 3, 4, 2) if swap else b.transpose(0, 1, 3, 2, 4)   # [tile][lh][li][(nt, r) | (r, nt)]
    n = min(32, 16 * NT)
    b = b.reshape(b.shape[0], 64, (16 * NT) // n, n).astype(np.uint64)
    wts = (np.uint64(1) << (n - 1 - np.arange(n)).astype(np.uint64))
    assert cout == act.shape[-1]
    return (b * wts).sum(-1)                                    # [tile][lane][word]


def mask_words(mask, nt_tiles):
    raw = mask.cpu().numpy()
    if nt_tiles == 1:
        return raw.view(np.uint16).reshape(-1, 64, 1).astype(np.uint64)
    return raw.view(np.uint32).reshape(-1, 64, nt_tiles // 2).astype(np.uint64)


class Case(object):
    """One first block on the device: image, weights, statistics from the patch moments, BatchNorm constants, a gradient."""

    def __init__(self, shape, cout, bias, seed=0, scale=None, shift=None):
        from capsyolo_amd import _lib
        self.lib = _lib
        B, H, W = walk_shape() if shape == 'walk' else shape
        self.B, self.H, self.W, self.cout = B, H, W, cout
        d = dev()
        self.x = rnd((B, 3, H, W), 11 + seed).to(d)
        self.w = rnd((cout, 3, 3, 3), 12 + seed, 27 ** -0.5).to(d)
        self.bias = rnd((cout,), 13 + seed, 0.3).to(d) if bias else None
        self.g = rnd((B, H, W, cout), 14 + seed).to(d)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        stats = torch.zeros((COPIES, cout, 2), dtype=torch.float64, device=d)
        self.wsm = torch.empty((_lib.query('cy_conv1_3x3_stats_ws_floats', B, H),), device=d)
        _lib.call('cy_conv1_3x3_stats', _p(self.x), _p(self.w), _p(self.bias), _p(stats), _p(self.wsm), B, H, W, cout, self.st)
        off = _lib.query('cy_conv1_3x3_stats_m2_offset', B, H)
        self.m2 = self.wsm[off:off + 2048]
        s = stats.sum(0) / (B * H * W)
        mean, var = s[:, 0], (s[:, 1] - s[:, 0] ** 2).clamp_min(0)
        invstd = (var + 1e-5).rsqrt()
        gamma, beta = 1 + 0.2 * rnd((cout,), 15 + seed).double().to(d), 0.3 * rnd((cout,), 16 + seed).double().to(d)
        self.mean, self.invstd = mean.float(), invstd.float()
        self.scale = (gamma * invstd).float() if scale is None else scale.to(d)
        self.shift = (beta - mean * gamma * invstd).float() if shift is None else shift.to(d)

    def forward(self, entry, with_mask):
        """(activation, mask) of one of the two entry points."""
        B, H, W, cout, lib = self.B, self.H, self.W, self.cout, self.lib
        y = torch.full((B, H, W, cout), float('nan'), device=dev())
        mask = None
        if entry == 'cy_conv1_3x3_fwd':
            lib.call(entry, _p(self.x), _p(self.w), _p(self.bias), _p(y), None, _p(self.scale), _p(self.shift), SLOPE, B, H, W, cout, self.st)
        else:
            if with_mask:
                nb = lib.query('cy_conv1_signmask_bytes', B, H, W, cout)
                assert nb == B * H * W * cout // 8
                mask = torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev())
            lib.call(entry, _p(self.x), _p(self.w), _p(self.bias), _p(y), _p(self.scale), _p(self.shift), SLOPE, _p(mask), B, H, W, cout, self.st)
        return y, mask

    def z(self):
        """The layer's own z = conv(x) + bias as the recompute path forms it (the plain forward stores acc + bias)."""
        B, H, W, cout = self.B, self.H, self.W, self.cout
        z = torch.empty((B, H, W, cout), device=dev())
        self.lib.call('cy_conv1_3x3_fwd', _p(self.x), _p(self.w), _p(self.bias), _p(z), None, None, None, 1.0, B, H, W, cout, self.st)
        return z

    def backward(self, mask):
        """(dW, dgamma, dbeta, redc, red_out) of the one-pass backward: with the mask, or recomputing z (mask None)."""
        B, H, W, cout, lib, d = self.B, self.H, self.W, self.cout, self.lib, dev()
        redc = torch.zeros((COPIES, cout, 2), dtype=torch.float64, device=d)
        dW, dgamma, dbeta = torch.empty((cout, 27), device=d), torch.empty((cout,), device=d), torch.empty((cout,), device=d)
        red = torch.empty((cout, 2), dtype=torch.float64, device=d)
        ws = torch.empty((lib.query('cy_conv1_bn_bwd_wgrad_ws_floats', B, H, W, cout),), device=d)
        head = [_p(self.x), _p(self.w), _p(self.bias), _p(self.g)] + ([_p(mask)] if mask is not None else [])
        lib.call('cy_conv1_bn_bwd_onepass_mask' if mask is not None else 'cy_conv1_bn_bwd_onepass', *head, _p(self.scale), _p(self.shift),
                 _p(self.mean), _p(self.invstd), SLOPE, _p(self.m2), _p(redc), _p(dW), _p(dgamma), _p(dbeta), _p(red), _p(ws),
                 B, H, W, cout, self.st)
        torch.cuda.synchronize()
        return dW, dgamma, dbeta, redc, red


NAMES = ('dW', 'dgamma', 'dbeta', 'striped sum of d', 'red_out')


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('cout', [32, 64, 128])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_untouched_mask_content_and_backward_bit_identity(shape, cout, bias):
    c = Case(shape, cout, bias)
    NT = cout // 32
    y0, _ = c.forward('cy_conv1_3x3_fwd', False)
    y1, none = c.forward('cy_conv1_3x3_fwd_act_mask', False)
    y2, mask = c.forward('cy_conv1_3x3_fwd_act_mask', True)
    torch.cuda.synchronize()
    assert none is None and torch.equal(y0, y1) and torch.equal(y0, y2)                 # forward untouched, to the byte
    # ---- content and layout: bit == stored activation > 0 (randn data: |y| * slope is nowhere near the denormals)
    act = y0.cpu().numpy()
    assert np.isfinite(act).all() and 0.2 < (act > 0).mean() < 0.8                         # both values of the bit occur
    yb = (c.z().double() * c.scale.double() + c.shift.double()).cpu().numpy()              # the backward's y, exact in sign
    assert (yb != 0).all()
    want, got = pack_expected(yb, NT), mask_words(mask, NT)
    assert want.shape == got.shape and np.array_equal(want, got)
    flips = (yb > 0) != (act > 0)                    # elements stored with the other sign than the backward sees: only with a bias
    print(shape, cout, bias, 'elements whose stored activation has the other sign:', int(flips.sum()))
    assert bias or not flips.any()
    assert np.array_equal(pack_expected(np.where(flips, yb, act), NT), got)                # bit == stored activation > 0 elsewhere
    if NT > 1:
        assert not np.array_equal(pack_expected(yb, NT, swap=True), got)                   # mutation: (r, nt) swapped is another answer
    # ---- the backward against the recompute path
    ref, new = c.backward(None), c.backward(mask)
    for name, a, b in zip(NAMES, ref, new):
        assert torch.equal(a, b), name


@pytest.mark.parametrize('cout', [32, 64, 128])
def test_one_flipped_bit_moves_its_channels_sum(cout):
    """Mutation on the device side: the top bit of lane (li, lh) of tile t is element (r, nt) = (0, 0) -- pixel 4 lh of the tile,
    channel NT li.  Flipping it changes d of that one element between g and g * slope, so exactly that channel's sum of d moves, by
    (1 - slope) |g|, and every other channel's stays to the bit."""
    NT = cout // 32
    c = Case((2, 3, 32), cout, False, seed=3)
    _, mask = c.forward('cy_conv1_3x3_fwd_act_mask', True)
    base = c.backward(mask)
    tile, li, lh = 4, 5, 1
    words = mask.cpu().numpy().copy()
    bytes_per_word = {1: 2, 2: 4, 4: 8}[NT]
    first = (tile * 64 + lh * 32 + li) * bytes_per_word              # little endian: the top bit of the first word is in ...
    top = first + (1 if NT == 1 else 3)                              # ... its last byte (16-bit word) / byte 3 (first 32-bit word)
    was_set = bool(words[top] & 0x80)
    words[top] ^= 0x80
    flipped = c.backward(torch.from_numpy(words).to(dev()))
    ch = NT * li
    gval = float(c.g.reshape(-1, 32, cout)[tile, 4 * lh, ch])
    dsum = (flipped[4].double() - base[4].double())[:, 0].cpu().numpy()
    want = (1 - SLOPE) * gval * (-1.0 if was_set else 1.0)
    others = np.delete(dsum, ch)
    assert np.all(others == 0.0)
    # the sums are fp32 per lane (48 values of size ~1 here) before they become double: 48 * 2^-24 * 48 on a change of size ~1
    assert abs(dsum[ch] - want) <= 2e-4 * max(1.0, abs(gval)), (dsum[ch], want)
    assert not torch.equal(flipped[0], base[0])


@pytest.mark.parametrize('cout', [32, 64, 128])
def test_both_values_of_the_bit_and_the_sign_of_zero(cout):
    """Channels by c % 4: scale = 0 with shift = +0, scale = 0 with shift = -0 (y = +-0: the bit is 0, d = g * slope), shift hugely
    negative (all bits 0), shift hugely positive (all bits 1, d = g)."""
    ch = torch.arange(cout)
    scale = torch.where(ch % 4 < 2, torch.zeros(cout), torch.ones(cout))
    shift = torch.tensor([0.0, -0.0, -1e30, 1e30]).repeat(cout // 4)
    c = Case((2, 3, 32), cout, False, seed=5, scale=scale, shift=shift)
    y0, _ = c.forward('cy_conv1_3x3_fwd', False)
    y2, mask = c.forward('cy_conv1_3x3_fwd_act_mask', True)
    assert torch.equal(y0, y2)
    act = y0.cpu().numpy()
    assert (act[..., 0::4] == 0).all() and (act[..., 1::4] == 0).all() and (act[..., 2::4] < 0).all() and (act[..., 3::4] > 0).all()
    got = mask_words(mask, cout // 32)
    assert np.array_equal(pack_expected(act, cout // 32), got)
    bits = np.unpackbits(mask.cpu().numpy()).mean()
    assert bits == 0.25                                                                    # exactly the channels c % 4 == 3
    ref, new = c.backward(None), c.backward(mask)
    for name, a, b in zip(NAMES, ref, new):
        assert torch.equal(a, b), name
    # d = g * slope where the bit is 0 and g where it is 1: the sum of d per channel.  fp32 sums of at most 48 values per lane,
    # then doubles: 48 * 2^-24 of the sum of |d|
    g = c.g.double().reshape(-1, cout)
    f = torch.where((ch % 4 == 3).to(dev()), torch.ones(cout, dtype=torch.float64, device=dev()), torch.full((cout,), SLOPE, dtype=torch.float64, device=dev()))
    want, bound = (g * f).sum(0), 48 * 2.0 ** -24 * (g.abs() * f).sum(0)
    # (SLOPE itself is the fp32 0.1 on the device: relative 1.5e-8, far inside the bound)
    assert bool(((new[4][:, 0] - want).abs() <= bound + 1e-7 * want.abs()).all())


@pytest.mark.parametrize('bias', [False, True])
def test_whole_block_switch_on_equals_switch_off(bias):
    """FusedBackbone conv -> BatchNorm -> LeakyReLU at 64 x 64, batch 64 (2^18 pixels: the moments gate is open) with
    ops.CONV1_SIGNMASK on and off: the same activation and the same parameter gradients to the bit, without a conv bias and with
    one (HipConv2d's default, the headline model's)."""
    from capsyolo_amd import _lib, models, ops
    x = rnd((64, 3, 64, 64), 21).to(dev())
    g = rnd((64, 64, 64, 128), 22).to(dev())
    torch.manual_seed(7)
    conv0 = models.HipConv2d(3, 128, 3, 1, 1, bias)
    state = {k: v.clone() for k, v in conv0.state_dict().items()}

    def run(on):
        seq = models.FusedBackbone()
        seq.add_module('conv_1', models.HipConv2d(3, 128, 3, 1, 1, bias))
        seq.add_module('bn_1', models.HipBatchNorm2d(128))
        seq.add_module('relu_1', models.HipLeakyReLU(0.1))
        seq.conv_1.load_state_dict(state)
        seq.to(dev()).train()
        was, ops.CONV1_SIGNMASK = ops.CONV1_SIGNMASK, on
        _lib.TRACE = []
        try:
            assert ops.conv_plan(x.shape, 128, 3, 1, 1, True).conv1_signmask == on
            y = seq(x, nchw_in=True)
            y.backward(g)
            torch.cuda.synchronize()
            calls = list(_lib.TRACE)
        finally:
            _lib.TRACE = None
            ops.CONV1_SIGNMASK = was
        assert ('cy_conv1_bn_bwd_onepass_mask' in calls) == on and ('cy_conv1_bn_bwd_onepass' in calls) == (not on), calls
        assert ('cy_conv1_3x3_fwd_act_mask' in calls) == on
        return y.detach(), [(n, p.grad) for n, p in seq.named_parameters()]
    assert ops.CONV1_SIGNMASK is True
    y_on, g_on = run(True)
    y_off, g_off = run(False)
    assert torch.equal(y_on, y_off)
    assert [n for n, _ in g_on] == [n for n, _ in g_off] and len(g_on) == (4 if bias else 3)
    for (n, a), (_, b) in zip(g_on, g_off):
        assert torch.equal(a, b), n


def test_plan_and_argument_checks():
    """The plan opens the mask exactly where the one-pass backward and the moments gate are open; the entry points refuse what
    their neighbours refuse."""
    from capsyolo_amd import _lib, ops
    big, small = (32, 3, 416, 416), (2, 3, 32, 32)
    assert ops.conv_plan(big, 128, 3, 1, 1, True).conv1_signmask and not ops.conv_plan(small, 128, 3, 1, 1, True).conv1_signmask
    for sw in ('CONV1_SIGNMASK', 'USE_CONV1_ONEPASS', 'USE_CONV1_MOMENTS', 'USE_CONV1_BWD', 'USE_CONV1'):
        was = getattr(ops, sw)
        setattr(ops, sw, False)
        try:
            assert not ops.conv_plan(big, 128, 3, 1, 1, True).conv1_signmask, sw
        finally:
            setattr(ops, sw, was)
    assert _lib.query('cy_conv1_signmask_bytes', 32, 416, 416, 128) == 32 * 416 * 416 * 16
    assert _lib.query('cy_conv1_signmask_bytes', 1, 1, 33, 128) == -1 and _lib.query('cy_conv1_signmask_bytes', 1, 1, 32, 48) == -1
    c = Case((1, 1, 32), 32, False)
    y = torch.empty((1, 1, 32, 32), device=dev())
    mask = torch.empty((128 + 16,), dtype=torch.uint8, device=dev())
    args = lambda m, slope=SLOPE, W=32: (_p(c.x), _p(c.w), None, _p(y), _p(c.scale), _p(c.shift), slope, m, 1, 1, W, 32, c.st)
    for bad, text in ((args(C.c_void_p(mask.data_ptr() + 4)), '16-byte aligned'), (args(_p(mask), slope=1.5), 'slope in [0, 1]'),
                      (args(_p(mask), W=48), 'multiple of 32')):
        with pytest.raises(_lib.HipExtensionError, match=text.replace('[', r'\[').replace(']', r'\]')):
            _lib.call('cy_conv1_3x3_fwd_act_mask', *bad)
    with pytest.raises(_lib.HipExtensionError, match='mask is NULL'):
        _lib.call('cy_conv1_bn_bwd_onepass_mask', _p(c.x), _p(c.w), None, _p(c.g), None, _p(c.scale), _p(c.shift), _p(c.mean), _p(c.invstd),
                  SLOPE, _p(c.m2), _p(y), _p(y), _p(y), _p(y), None, _p(y), 1, 1, 32, 32, c.st)

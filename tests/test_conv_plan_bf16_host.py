"""The bf16 convolution's plan (ops.conv_plan_bf16): whether the bf16 kernels are built for a layer, how its input gradient goes out
and what its block may fuse.  Host arithmetic: no GPU.  The rows of BASELINE configs[4] (the darkcapsule backbone behind its first
block) are pinned literally, taken from the conditions this function replaced; a change of any of them is a change of which kernel
runs a measured configuration and has to be made here on purpose."""
import itertools

import pytest

from helpers import REPO  # noqa: F401  (puts the repository on sys.path)

from capsyolo_amd import ops

FLAGS = ('ok', 'dgrad_one_launch', 'dgrad_bn_fuse', 'dgrad_premasks', 'wgrad_bn')
SWITCHES = ('BF16_DGRAD_ONE_LAUNCH', 'FUSE_BN_BWD_REDUCE_BF16', 'FUSE_BN_BWD_APPLY_BF16')
FAMILIES = ('conv_bf16_fwd', 'conv_bf16_dgrad', 'conv_bf16_wgrad')


def row(*args, **kw):
    """(forward, input gradient, weight gradient, names of the facts that hold, forward launches, input-gradient launches)."""
    p = ops.conv_plan_bf16(*args, **kw)
    return (p.fwd, p.dgrad, p.wgrad, ' '.join(f for f in FLAGS if getattr(p, f)), len(p.launches['fwd']), len(p.launches['dgrad']))


def test_switch_defaults():
    """The rows below are the plans of the DEFAULT switches."""
    assert all(getattr(ops, s) is True for s in SWITCHES)


# ------------------------------------------------------------------------------------------------ the measured configuration
S1 = FAMILIES + ('ok dgrad_bn_fuse dgrad_premasks wgrad_bn', 1, 1)                     # stride 1: ONE parity class, nothing to join
S2 = FAMILIES + ('ok dgrad_one_launch dgrad_bn_fuse dgrad_premasks wgrad_bn', 1, 1)    # stride 2, even map: four classes in one launch


def darkcaps_rows(H, B):
    """conv_2 .. conv_5 of models._darkcaps_backbone as FusedBackbone._forward_bf16 configures them: conv_1 has a BatchNorm and so
    hands its activation over as bf16 (in_f32 stays False for conv_2; its plan allows the fused sums, and the block then finds no
    hand-over to give them to), conv_5 writes fp32 for the routing head."""
    return [row((B, H, H, 128), 256, 3, 1, 1, in_f32=False), row((B, H, H, 256), 64, 4, 2, 1), row((B, H // 2, H // 2, 64), 128, 4, 2, 1),
            row((B, H // 4, H // 4, 128), 256, 4, 2, 1, out_f32=True)]


@pytest.mark.parametrize('H,B', [(608, 32), (608, 2), (96, 8)])
def test_darkcapsule_bf16_backbone_keeps_its_plan(H, B):
    assert darkcaps_rows(H, B) == [S1, S2, S2, S2]


def test_an_fp32_producer_takes_no_fused_sums():
    """A first block without BatchNorm hands fp32 over: the input gradient leaves in fp32 and sums nothing."""
    assert row((2, 96, 96, 128), 256, 3, 1, 1, in_f32=True) == FAMILIES + ('ok wgrad_bn', 1, 1)
    assert row((2, 96, 96, 128), 256, 4, 2, 1, in_f32=True) == FAMILIES + ('ok dgrad_one_launch wgrad_bn', 1, 1)


def test_odd_map_goes_out_class_by_class():
    """4x4 / stride 2 over a 9 x 32 map: the parity classes differ in size (5 and 4 rows), so each gets its own launch although
    BF16_DGRAD_ONE_LAUNCH is on; the even map next to it takes one."""
    odd = ops.conv_plan_bf16((2, 9, 32, 128), 128, 4, 2, 1)
    assert odd.ok and not odd.dgrad_one_launch and len(odd.launches['dgrad']) == 4 and len(odd.launches['fwd']) == 1
    even = ops.conv_plan_bf16((2, 8, 32, 128), 128, 4, 2, 1)
    assert even.ok and even.dgrad_one_launch and len(even.launches['dgrad']) == 1
    assert sum(p['ntiles'] for p in odd.launches['dgrad']) == 4          # (2 * 5 * 16 pixels and below: one 512 x 128 tile per class)
    assert even.launches['dgrad'][0]['ntiles'] == 4
    # conv_bf16_plans hands out the same lists by pass
    assert ops.conv_bf16_plans('dgrad', (2, 9, 32, 128), 128, 4, 2, 1) == odd.launches['dgrad']
    assert ops.conv_bf16_plans('fwd', (2, 9, 32, 128), 128, 4, 2, 1) == odd.launches['fwd']


# ------------------------------------------------------------------------------------------------ ok against the retired predicate
GEOMETRIES = [(3, 1, 1), (4, 2, 1), (3, 1, 0), (3, 2, 1), (4, 2, 0), (1, 1, 0), (5, 1, 2)]
CHANNELS = [32, 64, 96, 128, 192, 256]


def retired_predicate(k, stride, pad, cin, cout):
    """The hand-written layer test of ops.py as it stood when conv_plan_bf16 replaced it (FusedBackbone._forward_bf16 was its
    only caller)."""
    return pad == 1 and ((k == 3 and stride == 1 and cout % 128 == 0) or (k == 4 and stride == 2)) and cin % 64 == 0 and cout % 64 == 0


def grid():
    for (k, s, p), cin, cout in itertools.product(GEOMETRIES, CHANNELS, CHANNELS):
        yield k, s, p, cin, cout


def test_ok_is_the_retired_predicate():
    n = 0
    for k, s, p, cin, cout in grid():
        for shape in ((2, 8, 32, cin), (2, 9, 33, cin)):
            assert ops.conv_plan_bf16(shape, cout, k, s, p).ok == retired_predicate(k, s, p, cin, cout), (shape, cout, k, s, p)
            n += 1
    assert n == 7 * 6 * 6 * 2


# ------------------------------------------------------------------------------------------------ switches, one at a time
# switch -> (the field it moves, a layer on which it does, the field's value with the switch on / off)
SWITCH_FIELD = {
    'BF16_DGRAD_ONE_LAUNCH': ('dgrad_one_launch', ((2, 8, 32, 128), 128, 4, 2, 1)),
    'FUSE_BN_BWD_REDUCE_BF16': ('dgrad_bn_fuse', ((2, 8, 32, 128), 128, 4, 2, 1)),
    'FUSE_BN_BWD_APPLY_BF16': ('wgrad_bn', ((2, 8, 32, 128), 128, 4, 2, 1)),
}
FOLLOWS = {'dgrad_bn_fuse': ('dgrad_premasks',)}      # the bf16 epilogue always stores the premasked gradient with the sums


@pytest.mark.parametrize('switch', SWITCHES)
def test_one_switch_off(switch, monkeypatch):
    """Exactly the named field moves (dgrad_premasks with dgrad_bn_fuse), and the plan follows the switch at the next call."""
    field, args = SWITCH_FIELD[switch]
    on = ops.conv_plan_bf16(*args)
    monkeypatch.setattr(ops, switch, False)
    off = ops.conv_plan_bf16(*args)
    moved = [f for f in on._fields if getattr(on, f) != getattr(off, f)]
    want = [field] + list(FOLLOWS.get(field, ()))
    if field == 'dgrad_one_launch':
        want.append('launches')                                      # four launches of one class each instead of one of four
        assert len(off.launches['dgrad']) == 4 and off.launches['fwd'] == on.launches['fwd']
    assert sorted(moved) == sorted(want), (switch, on, off)
    assert getattr(on, field) is True and getattr(off, field) is False
    monkeypatch.setattr(ops, switch, True)
    assert ops.conv_plan_bf16(*args) == on


def test_every_switch_is_covered():
    assert sorted(SWITCH_FIELD) == sorted(SWITCHES)
    bf16_conv = [n for n in dir(ops) if n.isupper() and (n.endswith('_BF16') or n == 'BF16_DGRAD_ONE_LAUNCH')]
    assert sorted(bf16_conv) == sorted(SWITCHES)


# ------------------------------------------------------------------------------------------------ invariants over the grid
@pytest.mark.parametrize('off', [None] + list(SWITCHES))
def test_invariants(off, monkeypatch):
    if off is not None:
        monkeypatch.setattr(ops, off, False)
    n = 0
    for (k, s, p, cin, cout), shape, in_f32, out_f32 in itertools.product(grid(), [(2, 8, 32), (1, 9, 33)], [False, True], [False, True]):
        pl = ops.conv_plan_bf16(shape + (cin,), cout, k, s, p, in_f32, out_f32)
        at = (off, shape, cin, cout, k, s, p, in_f32, out_f32, pl)
        assert pl.dgrad_premasks == pl.dgrad_bn_fuse, at
        assert not (pl.dgrad_bn_fuse and in_f32), at
        assert not pl.wgrad_bn or pl.ok, at
        assert (pl.fwd, pl.dgrad, pl.wgrad) == (FAMILIES if pl.ok else (None, None, None)), at
        assert all(type(getattr(pl, f)) is bool for f in FLAGS), at
        n += 1
    assert n == 7 * 6 * 6 * 2 * 2 * 2


def test_plan_is_immutable():
    pl = ops.conv_plan_bf16((2, 8, 32, 128), 128, 4, 2, 1)
    with pytest.raises(AttributeError):
        pl.ok = False

"""What travels between two conv blocks (ops.BnHandover) and what does not (ops.ConvBlockCfg): the give / take protocol of the
BatchNorm-backward sums, and a cfg that is static.  Host logic: no GPU."""
import pytest

from helpers import REPO  # noqa: F401  (puts the repository on sys.path)

from capsyolo_amd import ops


def test_handover_gives_once_and_takes_once():
    h = ops.BnHandover('scale', 'shift', 'mean', 'invstd', 0.1)
    assert (h.z, h.scale, h.shift, h.mean, h.invstd, h.slope) == (None, 'scale', 'shift', 'mean', 'invstd', 0.1)
    assert h.take_red() is None                      # nobody gave any: the producer sums for itself
    h.give_red('red', 1)
    assert h.take_red() == ('red', True)             # the pair, premasked as a bool
    assert h.take_red() is None                      # ... exactly once
    h.give_red('again', False)
    assert h.take_red() == ('again', False) and h.take_red() is None
    assert ops.BnHandover(1, 2, 3, 4, 1, z='z').z == 'z'
    with pytest.raises(AttributeError):
        h.red = 'no attribute outside the protocol'  # __slots__


def test_cfg_is_static_and_carries_no_handover():
    cfg = ops.ConvBlockCfg(3, 1, 1, True, None, 0.1, 'c', defer_act=True)
    assert sorted(vars(cfg)) == sorted(['k', 'stride', 'pad', 'nchw_in', 'bn', 'slope', 'name', 'defer_act', 'out_bf16', 'in_f32', 'out_f32'])
    assert not any(hasattr(cfg, a) for a in ('in_holder', 'out_holder', 'holder', 'in_slope'))
    assert (cfg.out_bf16, cfg.in_f32, cfg.out_f32) == (False, False, False)
    with pytest.raises(TypeError):
        ops.ConvBlockCfg(3, 1, 1, in_slope=0.1)

"""GPU tests of csrc/loss.hip behind capsyolo_amd.loss_fns on the case table of tests/loss_cases.py (validated on the CPU by
tests/test_loss_cases_host.py).  The yardstick is oracle/loss_fns.py in fp64; the tolerances are those of test_losses_golden.
Every gradient is compared as a whole: before the forward and before the backward the allocator's free blocks are filled with NaN,
so an element that a kernel does not write shows as a NaN the reference does not have."""
import numpy as np
import pytest
import torch

import loss_cases as L
from capsyolo_amd import loss_fns
from capsyolo_amd._lib import HipExtensionError
from helpers import make_params

pytestmark = pytest.mark.gpu


def _poison(case):
    """Blocks of the sizes the loss allocates (the gradient of every differentiable input, the scalars), filled with NaN and freed:
    torch.empty hands them out again as they are."""
    def fill():
        held = [torch.full(case['inputs'][n].shape, float('nan'), device='cuda') for n in case['diff'] for _ in range(2)]
        held += [torch.full((), float('nan'), device='cuda') for _ in range(4)]
        torch.cuda.synchronize()
        del held
    return fill


def _run(name):
    case = L.CASES[name]
    fill = _poison(case)
    fill()
    return L.run(case, loss_fns, torch.float32, 'cuda', before_backward=fill)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', L.names())
def test_loss_case(name):
    case = L.CASES[name]
    got = _run(name)
    fr = L.fractions(case['kind'], got, L.reference(name))
    print('%s: error / tolerance %s' % (name, dict((k, '%.3g' % v) for k, v in fr.items())))
    L.compare(case['kind'], got, L.reference(name))
    for g in got['grad'].values():
        assert g.dtype == np.float32
    # the file header promises a fixed summation order: a second run gives the same bits
    again = _run(name)
    assert _same_bits(got['loss'], again['loss'])
    for k, g in got['grad'].items():
        assert _same_bits(g, again['grad'][k]), k
    if case['kind'] == 'dark':
        assert _same_bits(got['avg_iou'], again['avg_iou'])


def test_hand_built_case_exact_parts():
    got = _run('dark/hand_built')
    g = got['grad']['y_pred'].reshape(4, 10)
    yp = L.CASES['dark/hand_built']['inputs']['y_pred'].reshape(4, 10)
    assert not g[2].any()                                               # the label that is neither 0 nor 1
    assert not g[0, 6:10].any() and g[0, 1:5].any()                     # the tie: box 0 is responsible
    assert not g[1, 6:10].any() and g[1, 1:5].any() and g[1, 0] == np.float32(2.0 * yp[1, 0])   # both IoU 0: box 0, target 0
    assert not g[3, 1:5].any() and g[3, 6:10].any()


def _cuda(shape, dtype=torch.float32):
    return torch.full(shape, 0.25, dtype=dtype, device='cuda')


def test_mis_shaped_arguments_are_refused(monkeypatch):
    """Every shape the kernels would walk past a buffer with: refused on the host.  None of them may reach a launch, so for the
    length of this test a call into the library is itself a failure."""
    from capsyolo_amd import ops

    def no_call(name, *args):
        raise AssertionError('%s was reached with mis-shaped arguments' % name)
    monkeypatch.setattr(ops, 'call', no_call)
    p = make_params(n_boxes=2, n_classes=3, n_grid=4, darknet_input=64, device='cuda')
    ok_pred, ok_true = (2, 4, 4, 13), (2, 4, 4, 8)
    for pred, true in [((2, 4, 4, 12), ok_true),            # fewer columns than 5 n_boxes + n_classes
                       ((2, 4, 4, 14), ok_true),
                       ((2, 4, 3, 13), (2, 4, 3, 8)),       # not a square grid
                       ((2, 4, 52), ok_true),
                       (ok_pred, (2, 4, 4, 48)),            # wide labels with classes
                       (ok_pred, (2, 4, 4, 5)),
                       (ok_pred, (2, 3, 3, 8)),             # another grid
                       (ok_pred, (1, 4, 4, 8)),
                       (ok_pred, (2, 16, 8))]:
        with pytest.raises(HipExtensionError, match='dark_loss'):
            loss_fns.dark_loss(_cuda(pred), _cuda(true, torch.float64), p)
    p0 = make_params(n_boxes=2, n_classes=0, n_grid=4, darknet_input=64, device='cuda')
    with pytest.raises(HipExtensionError, match='dark_loss'):
        loss_fns.dark_loss(_cuda((2, 4, 4, 10)), _cuda((2, 4, 4, 4), torch.float64), p0)      # fewer than five label columns
    with pytest.raises(HipExtensionError, match='dark_loss'):
        loss_fns.dark_loss(_cuda((2, 4, 4, 13)), _cuda((2, 4, 4, 5), torch.float64), p0)      # predictions with class columns
    for caps, y in [((2, 2, 2, 5), (2, 3, 3, 8)), ((2, 2, 2, 5), (1, 2, 2, 8)), ((2, 2, 2, 5), (2, 2, 2, 4)), ((2, 2, 2, 6), (2, 2, 2, 8)),
                    ((2, 4, 5), (2, 2, 2, 8))]:
        with pytest.raises(HipExtensionError, match='darkcapsule_loss'):
            loss_fns.darkcapsule_loss(_cuda(caps), _cuda(y, torch.float64), p)
    for caps, y in [((2, 2, 2, 8), (2, 3, 3, 8)), ((2, 2, 2, 8), (2, 2, 2, 7)), ((2, 2, 2, 8), (2, 4, 8)), ((2, 2, 2, 3, 8), (2, 2, 2, 8))]:
        with pytest.raises(HipExtensionError, match='darkcapsule2_loss'):
            loss_fns.darkcapsule2_loss(_cuda(caps), _cuda(y, torch.float64), p)
    for caps, y in [((2, 2, 2, 3, 9), (2, 3, 3, 8)), ((2, 2, 2, 3, 9), (2, 2, 2, 9)), ((2, 2, 2, 27), (2, 2, 2, 8)), ((2, 2, 2, 3, 9), (2, 4, 8))]:
        with pytest.raises(HipExtensionError, match='darkcapsule3_loss'):
            loss_fns.darkcapsule3_loss(_cuda(caps), _cuda(y, torch.float64), p)

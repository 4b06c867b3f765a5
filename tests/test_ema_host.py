"""CPU-side tests of optim.Adam's moving average of the parameters (cy_adam_step's ema_table in csrc/adam.hip): the constructor's argument checks,
the decay schedule, step_scalars, the unchanged state_dict, the C ABI, main.py's options, and the float64 reference of the GPU tests
(tests/ema_ref.py) against closed forms and on the recipe those tests use."""
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO

import capsyolo_amd  # noqa: F401
from capsyolo_amd import _lib, optim

import ema_ref
import test_gpu_adam as A

def test_the_four_exports():
    """The four steps with the average are cy_adam_step with an ema_table: one entry point of two arguments, whose descriptor carries
    ema_table and one_minus_decay (its field order: test_host_logic.test_ctypes_structs_match_header_field_order; that the eight
    entry points it replaced are gone: tests/test_adam_step_host.py)."""
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    decl = re.search(r'\bint cy_adam_step\(([^;]*)\);', header, re.S)
    assert decl, 'cy_adam_step is not declared in capsyolo_hip.h'
    args = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S)
    assert len(args.split(',')) == 2 and 'cy_adam_step_t' in args
    assert 'cy_adam_step' in _lib.EXPORTS and hasattr(lib, 'cy_adam_step') and len(_lib._SIGS['cy_adam_step']) == 2
    body = re.search(r'typedef struct \{([^{}]*)\}\s*cy_adam_step_t;', header, re.S).group(1)
    assert 'ema_table' in body and 'one_minus_decay' in body
    assert set(['ema_table', 'one_minus_decay']) <= set(f[0] for f in _lib.AdamStep._fields_)
    assert lib.capsyolo_abi_version() == _lib.ABI_VERSION == 6


@pytest.mark.parametrize('v', [True, False, 0, 1, 0.0, 1.0, -0.5, 1.5, float('inf'), float('nan'), '0.9', (0.9,)])
def test_ema_decay_must_be_inside_the_unit_interval(v):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match='ema_decay'):
        optim.Adam([p], lr=1e-3, ema_decay=v)


def test_ema_warmup_needs_a_decay():
    with pytest.raises(ValueError, match='ema_warmup'):
        optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, ema_warmup=True)


@pytest.mark.parametrize('decay', [0.9, 0.999, 0.9999])
def test_decay_schedule(decay):
    p = torch.nn.Parameter(torch.zeros(3))
    flat, warm = optim.Adam([p], ema_decay=decay), optim.Adam([p], ema_decay=decay, ema_warmup=True)
    assert all(flat.ema_decay_at(t) == decay for t in (1, 2, 10, 10 ** 6))
    assert warm.ema_decay_at(1) == 2.0 / 11.0 and warm.ema_decay_at(2) == 3.0 / 12.0
    # (1 + t) / (10 + t) >= D  <=>  t >= (10 D - 1) / (1 - D): 80 steps for 0.9, 8990 for 0.999, 89990 for 0.9999
    end = int(math.ceil((10.0 * decay - 1.0) / (1.0 - decay) - 1e-6))
    assert end == {0.9: 80, 0.999: 8990, 0.9999: 89990}[decay] == ema_ref.warmup_end(decay)
    assert warm.ema_decay_at(end - 1) == end / (9.0 + end) < decay
    assert warm.ema_decay_at(end) == decay == warm.ema_decay_at(end + 1)
    ds = [warm.ema_decay_at(t) for t in range(1, end + 2)]
    assert all(a <= b for a, b in zip(ds, ds[1:]))
    assert all(warm.ema_decay_at(t) == ema_ref.decay_at(decay, True, t) for t in (1, 7, end, end + 5))


def test_step_scalars_six_or_eight():
    p = torch.nn.Parameter(torch.zeros(3))
    off, on = optim.Adam([p], lr=2e-3), optim.Adam([p], lr=2e-3, ema_decay=0.999)
    warm = optim.Adam([p], lr=2e-3, ema_decay=0.999, ema_warmup=True)
    g = off.param_groups[0]
    s6, s8, w8 = off.step_scalars(g, 3), on.step_scalars(g, 3), warm.step_scalars(g, 3)
    assert len(s6) == 6 and len(s8) == 8 and len(w8) == 8
    assert s8[:6] == s6 == w8[:6] and s8[7] == 0.0 == w8[7]
    # 1 - decay in double, rounded to fp32 once on its way out: the nearest fp32 to 0.001, which 1.f - 0.999f is not
    assert s8[6] == 1.0 - 0.999
    assert np.float32(s8[6]) == np.float32(0.001) != np.float32(1.0) - np.float32(0.999)
    assert w8[6] == 1.0 - 4.0 / 13.0
    with pytest.raises(RuntimeError, match='ema_decay is off'):
        off.ema_decay_at(1)


def test_the_average_is_an_attribute_not_state():
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    plain = optim.Adam(ps, lr=2e-3, betas=(0.8, 0.9), eps=1e-6)
    avg = optim.Adam(ps, lr=2e-3, betas=(0.8, 0.9), eps=1e-6, ema_decay=0.99, ema_warmup=True)
    assert avg.ema_decay == 0.99 and avg.ema_warmup is True and avg.ema == {}
    assert plain.ema_decay is None and plain.ema_warmup is False and plain.ema == {}
    sd_plain, sd_avg = plain.state_dict(), avg.state_dict()
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))], lr=2e-3, betas=(0.8, 0.9), eps=1e-6)
    assert sorted(sd_avg) == sorted(ref.state_dict()) == ['param_groups', 'state']
    assert [sorted(g) for g in sd_avg['param_groups']] == [sorted(g) for g in sd_plain['param_groups']]
    assert set(sd_avg['param_groups'][0]) <= set(ref.state_dict()['param_groups'][0])
    assert sd_avg == sd_plain
    ref.load_state_dict(sd_avg)
    net = torch.nn.Linear(1, 1)
    with pytest.raises(RuntimeError, match='ema_decay is off'):
        with plain.ema_weights():
            pass
    with pytest.raises(RuntimeError, match='ema_decay is off'):
        plain.ema_state_dict(net)
    with pytest.raises(RuntimeError, match='ema_decay is off'):
        plain.load_ema_state_dict(net, {})


def test_ema_state_dict_names_and_frozen_parameters():
    """Keyed by the model's parameter names; a parameter without an average (frozen, or not stepped yet) contributes its own values;
    loading puts the entries of the optimizer's parameters back and leaves the others alone.  (Host tensors: no step is taken.)"""
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    net[0].weight.requires_grad = False
    opt = optim.Adam([p for p in net.parameters() if p.requires_grad], ema_decay=0.9)
    sd = opt.ema_state_dict(net)
    assert list(sd) == [n for n, _ in net.named_parameters()]
    assert all(torch.equal(sd[n], p) and sd[n].data_ptr() != p.data_ptr() for n, p in net.named_parameters())
    new = dict((n, v + 1.0) for n, v in sd.items())
    opt.load_ema_state_dict(net, new)
    assert set(opt.ema) == set(p for p in net.parameters() if p.requires_grad)
    back = opt.ema_state_dict(net)
    assert torch.equal(back['0.weight'], net[0].weight) and torch.equal(back['1.bias'], net[1].bias + 1.0)
    with pytest.raises(KeyError, match='1.bias'):
        opt.load_ema_state_dict(net, dict((n, v) for n, v in new.items() if n != '1.bias'))
    # the exchange: pointers, and back
    before = dict((n, (p.data_ptr(), p.detach().clone())) for n, p in net.named_parameters())
    with opt.ema_weights():
        assert torch.equal(net[1].bias, before['1.bias'][1] + 1.0) and net[0].weight.data_ptr() == before['0.weight'][0]
        assert net[1].bias.data_ptr() != before['1.bias'][0]
        assert torch.equal(opt.ema_state_dict(net)['1.bias'], before['1.bias'][1] + 1.0)
        with pytest.raises(RuntimeError, match='ema_weights'):
            opt.step()
        with pytest.raises(RuntimeError, match='already inside'):
            opt.ema_weights().__enter__()
    assert all(p.data_ptr() == before[n][0] and torch.equal(p, before[n][1]) for n, p in net.named_parameters())


# ------------------------------------------------------------------------------------------------ the reference checks itself
def _run(ref, params, steps, grad):
    for t in range(1, steps + 1):
        for k, p in enumerate(params):
            p.grad = grad(k, t)
        ref.step()


def test_reference_constant_parameter():
    """Zero gradients: Adam does not move the parameter (m = v = 0), and the average of a constant is the constant, to the last bit
    for d * c + (1 - d) * c only where the two products round kindly, so within 2 ulp of double here."""
    p = torch.nn.Parameter(torch.tensor([0.3, -1.7, 5.0], dtype=torch.float64))
    start = p.detach().clone()
    ref = ema_ref.EmaRef([dict(params=[p], lr=1e-2)], 0.9, True, more=[(0.999, False)])
    _run(ref, [p], 12, lambda k, t: torch.zeros(3, dtype=torch.float64))
    assert torch.equal(p.detach(), start) and int(ref.state[p]['step']) == 12
    for tr in ref.trackers:
        assert float((tr.ema[p] - start).abs().max()) <= 12 * 2.0 ** -52 * 5.0


@pytest.mark.parametrize('warmup', [False, True])
def test_reference_closed_form_two_steps(warmup):
    """ema_2 = d_1 d_2 p_0 + (1 - d_1) d_2 p_1 + (1 - d_2) p_2 with the parameters torch.optim.Adam itself reaches."""
    p = torch.nn.Parameter(torch.tensor([1.0, -2.0], dtype=torch.float64))
    ref = ema_ref.EmaRef([dict(params=[p], lr=0.1)], 0.75, warmup)
    snaps = [p.detach().clone()]
    for t in (1, 2):
        p.grad = torch.tensor([0.5 * t, -1.0], dtype=torch.float64)
        ref.step()
        snaps.append(p.detach().clone())
    assert not torch.equal(snaps[0], snaps[1]) and not torch.equal(snaps[1], snaps[2])
    d1, d2 = (2.0 / 11.0, 3.0 / 12.0) if warmup else (0.75, 0.75)
    want = d1 * d2 * snaps[0] + (1 - d1) * d2 * snaps[1] + (1 - d2) * snaps[2]
    np.testing.assert_allclose(ref.ema[p].numpy(), want.numpy(), rtol=1e-14, atol=0)


def test_reference_on_the_recipe():
    """The recipe of the GPU tests over its 30 steps: it holds a step in which parameter 2 has no gradient and a non-finite step, and the
    reference treats them as the rule says: parameter 2's average keeps its bits where it has no gradient and follows its own count
    under the warm-up (20 steps after 30); the two poisoned steps move no average and count as skipped."""
    steps = range(1, ema_ref.STEPS + 1)
    lagging = [t for t in steps if not ema_ref.has_grad(2, t)]
    assert lagging == list(range(1, 31, 3)) and all(ema_ref.has_grad(k, t) for k in range(8) if k != 2 for t in steps)
    bad = [t for t in steps if any(not torch.isfinite(ema_ref.recipe_grad(k, t, poison=True)).all() for k in range(8) if ema_ref.has_grad(k, t))]
    assert bad == sorted(ema_ref.POISON) == [5, 11]
    assert all(torch.isfinite(ema_ref.recipe_grad(k, t)).all() for k in range(8) for t in (5, 11))

    ps = [torch.nn.Parameter(A._init(k).double()) for k in range(8)]
    ref = ema_ref.EmaRef([dict(params=ps[:4], **A.GROUPS[0]), dict(params=ps[4:], **A.GROUPS[1])], 0.999, True, None, True)
    by_hand, n2 = None, 0
    for t in steps:
        for k, q in enumerate(ps):
            q.grad = ema_ref.recipe_grad(k, t, poison=True).double() if ema_ref.has_grad(k, t) else None
        before = dict((q, v.clone()) for q, v in ref.ema.items())
        if by_hand is None and ema_ref.has_grad(2, t):
            by_hand = ps[2].detach().clone()
        ref.step()
        if t in ema_ref.POISON:
            assert all(torch.equal(before[q], ref.ema[q]) for q in before), t
        elif not ema_ref.has_grad(2, t):
            assert ps[2] not in before or torch.equal(before[ps[2]], ref.ema[ps[2]]), t
        if ema_ref.has_grad(2, t):
            n2 += 1
            if t not in ema_ref.POISON:
                d = min(0.999, (1.0 + n2) / (10.0 + n2))
                by_hand = d * by_hand + (1.0 - d) * ps[2].detach()
    assert ref.skipped == 2 and n2 == 20 == int(ref.state[ps[2]]['step']) and int(ref.state[ps[0]]['step']) == 30
    assert torch.equal(by_hand, ref.ema[ps[2]])


# ------------------------------------------------------------------------------------------------ main.py
def _main():
    spec = importlib.util.spec_from_file_location('cy_main', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_main_knows_the_options(tmp_path):
    m = _main()
    args = m.parser.parse_args(['--model', 'capsule', '--ema', '0.99', '--ema_warmup', '--use_ema'])
    assert args.ema == 0.99 and args.ema_warmup is True and args.use_ema is True
    args = m.parser.parse_args(['--model', 'capsule'])
    assert args.ema is None and args.ema_warmup is False and args.use_ema is False
    cfg = dict(batch_size=8, n_epochs=1, n_classes=43, lr_decay=0.1, capsule_input=32)
    json.dump(cfg, open(str(tmp_path / 'params.json'), 'w'))
    p = m.load_params(str(tmp_path), args)
    assert p.ema_decay is None and p.ema_warmup is False and p.use_ema is False
    json.dump(dict(cfg, ema_decay=0.999, ema_warmup=True), open(str(tmp_path / 'params.json'), 'w'))
    p = m.load_params(str(tmp_path), args)
    assert p.ema_decay == 0.999 and p.ema_warmup is True
    p = m.load_params(str(tmp_path), m.parser.parse_args(['--model', 'capsule', '--ema', '0.9']))
    assert p.ema_decay == 0.9 and p.ema_warmup is True                   # the command line wins


def test_main_refusals(tmp_path):
    m = _main()
    json.dump(dict(batch_size=8, n_epochs=1, n_classes=43, lr_decay=0.1, dropout=0.0), open(str(tmp_path / 'params.json'), 'w'))
    base = ['--model', 'cnn', '--cnn_kernels', 'torch', '--synthetic', '8', '--model_dir', str(tmp_path)]
    with pytest.raises(SystemExit, match="--ema needs the project's Adam"):
        m.main(base + ['--ema', '0.9'])
    for bad in ('0', '1', '1.5', 'nan'):
        with pytest.raises(SystemExit, match=r'decay in \(0, 1\)'):
            m.main(base + ['--ema', bad])
    with pytest.raises(SystemExit, match='give --ema D'):
        m.main(base + ['--ema_warmup'])
    with pytest.raises(SystemExit, match='--use_ema runs a restored model'):
        m.main(base + ['--use_ema'])


def test_load_checkpoint_with_and_without_the_entry(tmp_path):
    """utils.load_checkpoint: params.use_ema puts the checkpoint's averages into the parameters (buffers stay the checkpoint's); without
    the entry True is refused with the documented message and 'if_present' loads the plain weights; a checkpoint without the entry
    loads as before."""
    import types
    from capsyolo_amd import utils
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    net[1].running_mean.fill_(0.25)
    ema = dict((n, p.detach() + 1.0) for n, p in net.named_parameters())
    with_ema, without = str(tmp_path / 'a.pth.tar'), str(tmp_path / 'b.pth.tar')
    torch.save({'epoch': 1, 'state_dict': net.state_dict(), 'ema_state_dict': ema}, with_ema)
    torch.save({'epoch': 1, 'state_dict': net.state_dict()}, without)

    def fresh():
        return torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    a = fresh()
    utils.load_checkpoint(with_ema, a, types.SimpleNamespace(use_ema=True))
    assert all(torch.equal(p, ema[n]) for n, p in a.named_parameters()) and float(a[1].running_mean[0]) == 0.25
    for path, params in ((with_ema, types.SimpleNamespace(use_ema=False)), (with_ema, None), (without, types.SimpleNamespace()),
                         (without, types.SimpleNamespace(use_ema='if_present'))):
        b = fresh()
        utils.load_checkpoint(path, b, params)
        assert all(torch.equal(v, net.state_dict()[k]) for k, v in b.state_dict().items())
    with pytest.raises(utils.NoEmaInCheckpoint, match="has no 'ema_state_dict' entry"):
        utils.load_checkpoint(without, fresh(), types.SimpleNamespace(use_ema=True))
    # into an optimizer that keeps averages
    c = fresh()
    opt = optim.Adam(c.parameters(), ema_decay=0.9)
    utils.load_checkpoint(with_ema, c, None, None)
    assert opt.ema == {}
    ck = torch.load(with_ema, weights_only=False)
    ck['optim_dict'] = opt.state_dict()
    torch.save(ck, with_ema)
    utils.load_checkpoint(with_ema, c, None, opt)
    assert all(torch.equal(opt.ema[p], ema[n]) for n, p in c.named_parameters())
    assert all(torch.equal(p, net.state_dict()[n]) for n, p in c.named_parameters())

"""CPU-side tests of optim.Adam's gradient-norm clipping and non-finite guard (csrc/gradnorm.hip, cy_adam_step's record in csrc/adam.hip):
the C ABI, the constructor's argument checks, the unchanged state_dict, main.py's options, and the float64 reference of the GPU tests
(tests/clip_ref.py) against an independent restatement of the rule on the recipe those tests use."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO

import capsyolo_amd  # noqa: F401
from capsyolo_amd import _lib, optim

import clip_ref
import test_gpu_adam as A

NEW = {'cy_grad_sumsq_multi': 6, 'cy_grad_clip_finish': 7, 'cy_adam_step': 2}     # (the step that reads the record: tests/test_adam_step_host.py)


def test_the_four_exports():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name, n_args in NEW.items():
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, header, re.S)
        assert decl, '%s is not declared in capsyolo_hip.h' % name
        args = re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S)
        assert len(args.split(',')) == n_args, name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(_lib._SIGS[name]) == n_args, name
    assert lib.capsyolo_abi_version() == _lib.ABI_VERSION == 6


@pytest.mark.parametrize('v', [0, -1, float('inf'), float('nan')])
def test_max_grad_norm_must_be_positive_and_finite(v):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match='max_grad_norm'):
        optim.Adam([p], lr=1e-3, max_grad_norm=v)


def test_options_are_attributes_not_group_entries():
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    plain = optim.Adam(ps, lr=2e-3, betas=(0.8, 0.9), eps=1e-6)
    both = optim.Adam(ps, lr=2e-3, betas=(0.8, 0.9), eps=1e-6, max_grad_norm=0.5, skip_nonfinite=True)
    assert both.max_grad_norm == 0.5 and both.skip_nonfinite is True
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    assert both.clip_record is None and both.skipped_dev is None        # device state is made by the first step that needs it
    sd_plain, sd_both = plain.state_dict(), both.state_dict()
    assert [sorted(g) for g in sd_both['param_groups']] == [sorted(g) for g in sd_plain['param_groups']]
    assert sd_both == sd_plain
    o = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))], lr=1.0)
    o.load_state_dict(sd_both)
    assert o.param_groups[0]['lr'] == 2e-3 and tuple(o.param_groups[0]['betas']) == (0.8, 0.9)
    with pytest.raises(RuntimeError, match='grad_stats'):
        plain.grad_stats()
    assert both.grad_stats() == {'norm': 0.0, 'coef': 1.0, 'skipped': 0}


def _numpy_rule(steps, max_norm, skip_nonfinite, poison=None):
    """The rule written out in numpy float64, with nothing of torch.optim in it: parameters, exp_avg, exp_avg_sq, step counts, and per
    step (norm, coef)."""
    groups = [A.GROUPS[0]] * 4 + [A.GROUPS[1]] * 4
    p = [A._init(k).double().numpy().copy() for k in range(8)]
    m, v, n = [np.zeros_like(q) for q in p], [np.zeros_like(q) for q in p], [0] * 8
    log = []
    for t in range(1, steps + 1):
        g = dict((k, clip_ref.recipe_grad(k, t).double().numpy().copy()) for k in range(8) if clip_ref.has_grad(k, t))
        if poison and t in poison:
            k, i, val = poison[t]
            g[k].reshape(-1)[i] = val
        norm = math.sqrt(sum(float((x * x).sum()) for x in g.values()))
        coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
        log.append((norm, coef))
        for k, x in g.items():
            n[k] += 1
            if skip_nonfinite and not math.isfinite(norm):
                continue
            hp = dict(betas=(0.9, 0.999), eps=1e-8)
            hp.update(groups[k])
            b1, b2 = hp['betas']
            x = coef * x
            m[k] = b1 * m[k] + (1 - b1) * x
            v[k] = b2 * v[k] + (1 - b2) * x * x
            p[k] = p[k] - hp['lr'] / (1 - b1 ** n[k]) * m[k] / (np.sqrt(v[k]) / math.sqrt(1 - b2 ** n[k]) + hp['eps'])
    return p, m, v, n, log


@pytest.mark.parametrize('max_norm,guard', [(clip_ref.MAX_NORM, False), (clip_ref.MAX_NORM, True), (None, True)])
def test_clip_ref_is_the_rule(max_norm, guard):
    """clip_ref.ClipRef (clip_grad_norm_ + torch.optim.Adam in float64) against the rule written out in numpy, on the recipe of the GPU
    tests: 10 steps, two groups, parameter 2 without a gradient every third step, gradients x 50 on even steps.  With max_norm = 1.0
    the even steps clip and the odd ones do not; with the guard, the poisoned steps of test_gpu_clip.py change nothing but the step
    counts."""
    poison = {3: (0, 0, float('inf')), 5: (7, 70000, float('nan')), 6: (6, 16384, float('-inf'))} if guard else None
    ps = [torch.nn.Parameter(A._init(k).double()) for k in range(8)]
    ref = clip_ref.ClipRef([dict(params=ps[:4], **A.GROUPS[0]), dict(params=ps[4:], **A.GROUPS[1])], max_norm, guard)
    seen = []
    for t in range(1, 11):
        for k, q in enumerate(ps):
            q.grad = clip_ref.recipe_grad(k, t).double() if clip_ref.has_grad(k, t) else None
        if poison and t in poison:
            k, i, val = poison[t]
            ps[k].grad.view(-1)[i] = val
        before = [q.detach().clone() for q in ps]
        ref.step()
        seen.append((ref.norm, ref.coef))
        if poison and t in poison:
            assert all(torch.equal(a, b) for a, b in zip(before, ps))
    p, m, v, n, log = _numpy_rule(10, max_norm, guard, poison)
    for t, ((norm, coef), (norm_w, coef_w)) in enumerate(zip(seen, log), 1):
        if math.isfinite(norm_w):
            assert abs(norm - norm_w) <= 1e-12 * norm_w and abs(coef - coef_w) <= 1e-12, t
        else:
            assert not math.isfinite(norm), t
    if max_norm is not None:
        clipped = [t for t, (norm, coef) in enumerate(log, 1) if math.isfinite(norm) and coef < 1.0]
        free = [t for t, (norm, coef) in enumerate(log, 1) if math.isfinite(norm) and coef == 1.0]
        assert clipped == [t for t in range(2, 11, 2) if not (poison and t in poison)], log
        assert free == [t for t in range(1, 11, 2) if not (poison and t in poison)], log
        assert all(norm + 1e-6 <= max_norm for norm, coef in log if math.isfinite(norm) and coef == 1.0)
    assert ref.skipped == (3 if guard else 0)
    for k, q in enumerate(ps):
        st = ref.state[q]
        assert int(st['step']) == n[k] == (10 - (4 if k == 2 else 0)), k
        # (exp_avg adds terms of both signs: its float64 rounding errors scale with the operands, not with the result)
        for got, want in ((q.detach().numpy(), p[k]), (st['exp_avg'].numpy(), m[k]), (st['exp_avg_sq'].numpy(), v[k])):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13 * float(np.abs(want).max()))


def _main():
    spec = importlib.util.spec_from_file_location('cy_main', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_main_knows_the_two_options(tmp_path):
    import json
    m = _main()
    args = m.parser.parse_args(['--model', 'capsule', '--clip_norm', '0.5', '--skip_nonfinite'])
    assert args.clip_norm == 0.5 and args.skip_nonfinite is True
    args = m.parser.parse_args(['--model', 'capsule'])
    assert args.clip_norm is None and args.skip_nonfinite is False
    cfg = dict(batch_size=8, n_epochs=1, n_classes=43, lr_decay=0.1, capsule_input=32)
    json.dump(cfg, open(str(tmp_path / 'params.json'), 'w'))
    p = m.load_params(str(tmp_path), args)
    assert p.clip_norm is None and p.skip_nonfinite is False
    json.dump(dict(cfg, clip_norm=2.0, skip_nonfinite=True), open(str(tmp_path / 'params.json'), 'w'))
    p = m.load_params(str(tmp_path), args)
    assert p.clip_norm == 2.0 and p.skip_nonfinite is True
    p = m.load_params(str(tmp_path), m.parser.parse_args(['--model', 'capsule', '--clip_norm', '0.5']))
    assert p.clip_norm == 0.5 and p.skip_nonfinite is True              # the command line wins


def test_skip_nonfinite_needs_the_projects_adam(tmp_path):
    import json
    m = _main()
    json.dump(dict(batch_size=8, n_epochs=1, n_classes=43, lr_decay=0.1, dropout=0.0), open(str(tmp_path / 'params.json'), 'w'))
    with pytest.raises(SystemExit, match="needs the project's Adam"):
        m.main(['--model', 'cnn', '--cnn_kernels', 'torch', '--synthetic', '8', '--model_dir', str(tmp_path), '--skip_nonfinite'])
    with pytest.raises(SystemExit, match='positive finite'):
        m.main(['--model', 'cnn', '--cnn_kernels', 'torch', '--synthetic', '8', '--model_dir', str(tmp_path), '--clip_norm', '-1'])


def test_torch_cnn_baseline_clips_with_torch(tmp_path, monkeypatch):
    """--clip_norm on the plain-torch cnn path: torch.nn.utils.clip_grad_norm_ once per step, between backward() and step()."""
    import json
    m = _main()
    json.dump(dict(batch_size=8, n_epochs=1, n_classes=43, lr_decay=0.1, dropout=0.0), open(str(tmp_path / 'params.json'), 'w'))
    calls, real = [], torch.nn.utils.clip_grad_norm_

    def spy(parameters, max_norm, *a, **kw):
        parameters = list(parameters)
        assert all(p.grad is not None for p in parameters)
        calls.append(max_norm)
        total = real(parameters, max_norm, *a, **kw)
        assert math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in parameters)) <= max_norm * 1.001      # (fp32 gradients)
        return total
    monkeypatch.setattr(torch.nn.utils, 'clip_grad_norm_', spy)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    losses_tr, _ = m.main(['--model', 'cnn', '--cnn_kernels', 'torch', '--synthetic', '16', '--model_dir', str(tmp_path), '--fix_ckpt_dir',
                           '--no_metric', '--clip_norm', '0.001'])
    assert calls == [0.001, 0.001] and np.isfinite(losses_tr[0])

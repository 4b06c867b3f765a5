"""GPU tests of optim.Adam's moving average of the parameters: the four steps of cy_adam_step with an ema_table (csrc/adam.hip; host or device scalars x clip record or
none) against tests/ema_ref.py (the rule in float64 on the CPU around clip_ref.ClipRef; checked against closed forms in
tests/test_ema_host.py), the exchange `with opt.ema_weights()`, checkpoints, the captured step and main.py's options.  The recipe is
ema_ref's: the 8 tensors of tests/test_gpu_adam.py (sizes around the 16384-element chunk), two groups, 30 steps, the learning rate cut
after step 10, parameter 2 without a gradient in steps 1, 4, 7, ...  The averages are held to test_gpu_adam.py's rule (rtol 1e-5, atol
1e-6): 30 steps x 3 roundings x 2^-24 = 5.4e-6 relative of their own, on top of parameters that are within that rule of float64 and
that a convex combination does not amplify.

Measured on the MI355X: each test's docstring has its figures, DESIGN.md section 6q all of them."""
import collections
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, make_params, synth_images

from capsyolo_amd import optim

import clip_ref
import ema_ref
import test_gpu_adam as A

pytestmark = pytest.mark.gpu

CONFIGS = [(0.9, False), (0.9, True), (0.999, False), (0.999, True)]
CHECK_AT = (10, 30)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def _hand_over(k, g):
    """The gradient on the device as test_gpu_adam hands it over: tensor 6 (32768 elements) as a non-contiguous transpose."""
    if k == 6:
        gt = g.t().contiguous().cuda().t()
        assert not gt.is_contiguous()
        return gt
    return g.cuda()


def _set_hip_grads(t, hip, grad=A._grad, lag=True):
    for k, p in enumerate(hip):
        p.grad = _hand_over(k, grad(k, t)) if (not lag or ema_ref.has_grad(k, t)) else None


def _cut_lr(t, *opts):
    if t == ema_ref.LR_CUT_AFTER:
        for o in opts:
            for g in o.param_groups:
                g['lr'] *= 0.1


def _two_groups(hip, **kw):
    return optim.Adam([dict(params=hip[:4], **A.GROUPS[0]), dict(params=hip[4:], **A.GROUPS[1])], **kw)


def _state_bits(params, opt):
    out = []
    for p in params:
        st = opt.state.get(p) or {}
        out.append([_bits(p)] + [_bits(st[k]) for k in ('exp_avg', 'exp_avg_sq') if k in st])
    return out


def _ema_bits(params, opt):
    return [_bits(opt.ema[p]) if p in opt.ema else None for p in params]


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(a, b))


def _fraction(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    return float(((got - want).abs() / (A.ATOL + A.RTOL * want.abs())).max())


@functools.lru_cache(maxsize=None)
def _reference(guard=False):
    """ONE float64 run of the recipe for every test that needs it: {(decay, warmup): {step: [average of parameter k]}}, the parameters at
    the same steps, parameter 2 after each of its updates, and the reference itself.  guard: skip_nonfinite with ema_ref.POISON."""
    ps = [torch.nn.Parameter(A._init(k).double()) for k in range(8)]
    ref = ema_ref.EmaRef([dict(params=ps[:4], **A.GROUPS[0]), dict(params=ps[4:], **A.GROUPS[1])], *CONFIGS[0], None, guard, more=CONFIGS[1:])
    emas, params, p2 = dict((c, {}) for c in CONFIGS), {}, [(0, ps[2].detach().clone())]
    for t in range(1, ema_ref.STEPS + 1):
        for k, q in enumerate(ps):
            q.grad = ema_ref.recipe_grad(k, t, poison=guard).double() if ema_ref.has_grad(k, t) else None
        ref.step()
        if ema_ref.has_grad(2, t):
            p2.append((t, ps[2].detach().clone()))
        if t in CHECK_AT:
            params[t] = [q.detach().clone() for q in ps]
            for c, tr in zip(CONFIGS, ref.trackers):
                emas[c][t] = [tr.ema[q].clone() for q in ps]
        _cut_lr(t, ref)
    return {'ema': emas, 'params': params, 'p2': p2, 'ref': ref, 'ps': ps}


# ------------------------------------------------------------------------------------------------ 1. the step is undisturbed
def _thirty_steps(dev, clip, ema_decay):
    """Parameters, exp_avg and exp_avg_sq after the 30 steps, and the entry points called.  dev: the device-scalar kernels, launched eagerly
    with graph_step.GraphedStep's tables from step 2 on (one group, a gradient for every parameter: the captured path takes nothing else);
    clip: max_grad_norm = 1.0 on clip_ref's gradients, which clip on even steps and do not on odd ones."""
    from capsyolo_amd import _lib
    _, hip = A._params(range(8))
    kw = dict(max_grad_norm=clip_ref.MAX_NORM) if clip else {}
    if ema_decay is not None:
        kw['ema_decay'] = ema_decay
    opt = optim.Adam(hip, **dict(A.GROUPS[1], **kw)) if dev else _two_groups(hip, **kw)
    grad = clip_ref.recipe_grad if clip else A._grad
    group = opt.param_groups[0]
    hyper = torch.zeros(len(opt.step_scalars(group, 1)), dtype=torch.float32, device='cuda')
    _lib.TRACE = trace = []
    try:
        for t in range(1, ema_ref.STEPS + 1):
            _set_hip_grads(t, hip, grad, lag=not dev)
            if dev and t == 2:                                           # after one eager step (it built the block map)
                opt.graph_hyper = {id(group): hyper}
                opt.graph_tables = {id(group): (torch.empty((8, 5), dtype=torch.int64).pin_memory(), torch.empty((8, 5), dtype=torch.int64, device='cuda'))}
                if ema_decay is not None:
                    opt.graph_ema_tables = {id(group): (torch.empty(8, dtype=torch.int64).pin_memory(), torch.empty(8, dtype=torch.int64, device='cuda'))}
            if dev and t >= 2:
                hyper.copy_(torch.tensor(opt.step_scalars(group, t), dtype=torch.float32))
            opt.step()
            torch.cuda.synchronize()
            _cut_lr(t, opt)
    finally:
        _lib.TRACE = None
        opt.graph_hyper, opt.graph_tables, opt.graph_ema_tables = None, None, None
    return hip, opt, trace


@pytest.mark.parametrize('dev', [False, True], ids=['host_scalars', 'device_scalars'])
@pytest.mark.parametrize('clip', [False, True], ids=['plain', 'clip'])
def test_the_step_is_undisturbed(dev, clip):
    """For each of the four kernel pairs: parameters, exp_avg and exp_avg_sq after 30 steps with ema_decay = 0.999 have the bits of the run
    with ema_decay = None, the run with the average goes through the _ema entry point and the run without it through the entry point
    it always went through; without the option no EMA tensor or table exists."""
    name = 'cy_adam_step' + ('+dev' if dev else '') + ('+clip' if clip else '')
    p_off, o_off, tr_off = _thirty_steps(dev, clip, None)
    p_on, o_on, tr_on = _thirty_steps(dev, clip, 0.999)
    n_first = 1 if dev else 0                                            # the eager first step of the device-scalar runs
    launches = sum(1 for n in tr_off if n.startswith('cy_adam_step'))
    assert launches == (30 if dev else 2 * 30 + 20)                      # two groups, and a third launch in parameter 2's 20 steps (it lags)
    assert tr_off.count(name) == launches - n_first and tr_on.count(name + '+ema') == launches - n_first
    assert not any(n.endswith('+ema') for n in tr_off) and [n.replace('+ema', '') for n in tr_on] == tr_off
    assert o_off.ema == {} and getattr(o_off, '_ema_table_dev', None) is None and getattr(o_off, '_ema_ring', None) is None
    # (parameter 0 is one element whose gradient is the recipe's exact zero: it never moves, and neither does its average)
    assert set(o_on.ema) == set(p_on) and all(not torch.equal(o_on.ema[p], p) for p in p_on[1:]) and torch.equal(o_on.ema[p_on[0]], p_on[0])
    assert _same([b for s in _state_bits(p_off, o_off) for b in s], [b for s in _state_bits(p_on, o_on) for b in s])
    assert all(int(o_on.state[a]['step']) == int(o_off.state[b]['step']) for a, b in zip(p_on, p_off))


# ------------------------------------------------------------------------------------------------ 2. the average is right
@pytest.mark.parametrize('decay,warmup', CONFIGS)
def test_the_average_against_float64(decay, warmup):
    """The averages of the 8 tensors against ema_ref at steps 10 and 30 (cy_adam_step+ema, two groups, parameter 2 lagging).
    Measured on the MI355X (largest error / tolerance over the 8 tensors, step 10 / step 30): 0.25 / 0.55 (0.9), 0.51 / 0.56 (0.9 with the
    warm-up), 0.04 / 0.06 (0.999), 0.51 / 0.56 (0.999 with the warm-up); the parameters themselves 0.56 / 0.56 (the fp32 1 - beta2 of
    DESIGN.md section 6n)."""
    want = _reference()
    _, hip = A._params(range(8))
    opt = _two_groups(hip, ema_decay=decay, ema_warmup=warmup)
    worst = {}
    for t in range(1, ema_ref.STEPS + 1):
        _set_hip_grads(t, hip)
        opt.step()
        if t in CHECK_AT:
            worst[t] = max(_fraction(opt.ema[p], want['ema'][(decay, warmup)][t][k]) for k, p in enumerate(hip))
            worst['param %d' % t] = max(_fraction(p, want['params'][t][k]) for k, p in enumerate(hip))
        _cut_lr(t, opt)
    print('ema_decay %g, warmup %s: largest error / tolerance %s' % (decay, warmup, dict((k, '%.3g' % v) for k, v in worst.items())))
    assert max(worst[t] for t in CHECK_AT) <= 1.0, worst


def test_the_rule_in_fp32_on_the_cpu_meets_the_tolerance():
    """The companion of the test above: torch.optim.Adam and the rule in fp32 torch on the CPU stay within the tolerance of the float64
    reference, so the tolerance is one that fp32 arithmetic can meet: at most 0.34 of it (0.999, step 30), otherwise at most 0.11.  (No kernel of the project runs here; it sits in this file because
    it shares the reference run.)"""
    want = _reference()
    ps = [torch.nn.Parameter(A._init(k)) for k in range(8)]
    opt = torch.optim.Adam([dict(params=ps[:4], **A.GROUPS[0]), dict(params=ps[4:], **A.GROUPS[1])])
    trackers = [ema_ref.EmaTracker(*c) for c in CONFIGS]
    worst = {}
    for t in range(1, ema_ref.STEPS + 1):
        live = [q for k, q in enumerate(ps) if ema_ref.has_grad(k, t)]
        for k, q in enumerate(ps):
            q.grad = A._grad(k, t) if ema_ref.has_grad(k, t) else None
        for tr in trackers:
            tr.before_step(live)
        opt.step()
        for q in live:
            for tr in trackers:
                tr.after_update(q, int(opt.state[q]['step']))
        if t in CHECK_AT:
            for c, tr in zip(CONFIGS, trackers):
                assert all(tr.ema[q].dtype == torch.float32 for q in ps)
                worst[c + (t,)] = max(_fraction(tr.ema[q], want['ema'][c][t][k]) for k, q in enumerate(ps))
        _cut_lr(t, opt)
    print('fp32 torch on the CPU: largest error / tolerance %s' % dict((k, '%.3g' % v) for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 3. lagging and missing gradients
def test_a_parameter_without_a_gradient_keeps_its_average():
    """ema_decay = 0.999 with the warm-up (in force for all 30 steps): the average of parameter 2 does not exist before its first step (step
    2), keeps its bits across each later step in which it has no gradient and moves in every other; after 30 steps it has taken 20 and
    its average is the reference's, whose d_t follows the parameter's OWN count: the same rule fed the global step count misses the
    tolerance by far (asserted, so that the comparison can tell the two apart).  Measured on the MI355X: 0.24 of the tolerance against
    its own count, 373 times the tolerance for the global count."""
    want = _reference()
    _, hip = A._params(range(8))
    opt = _two_groups(hip, ema_decay=0.999, ema_warmup=True)
    for t in range(1, ema_ref.STEPS + 1):
        _set_hip_grads(t, hip)
        before = _ema_bits(hip, opt)
        opt.step()
        after = _ema_bits(hip, opt)
        if t == 1:
            assert before == [None] * 8 and after[2] is None and hip[2] not in opt.ema
        if not ema_ref.has_grad(2, t):
            assert _same([before[2]], [after[2]]), 'step %d moved the average of parameter 2' % t
        elif t > 2:
            assert not torch.equal(before[2], after[2]), t
        assert all(b is None or not torch.equal(b, a) for k, (b, a) in enumerate(zip(before, after)) if k not in (0, 2)), t   # (0: a zero gradient)
        _cut_lr(t, opt)
    assert int(opt.state[hip[2]]['step']) == 20 and int(opt.state[hip[0]]['step']) == 30
    right = want['ema'][(0.999, True)][30][2]
    wrong = want['p2'][0][1].clone()
    for t_global, p in want['p2'][1:]:
        d = ema_ref.decay_at(0.999, True, t_global)
        wrong = d * wrong + (1.0 - d) * p
    got, off = _fraction(opt.ema[hip[2]], right), _fraction(wrong, right)
    print('parameter 2: error / tolerance %.3g against its own count, %.3g for the rule on the global count' % (got, off))
    assert got <= 1.0 and off > 10.0


# ------------------------------------------------------------------------------------------------ 4. skip
def test_a_skipped_step_moves_no_average():
    """skip_nonfinite with one gradient element inf in step 5 and one NaN in step 11 (cy_adam_step+clip+ema: record[2] == 0 returns before
    anything is read or written): every average, parameter, exp_avg and exp_avg_sq keeps its bits across the two steps, skipped counts 2,
    and averages and state after 30 steps are the reference's.  Measured on the MI355X: averages 0.47 of the tolerance, parameters /
    exp_avg / exp_avg_sq 0.53 / 0.13 / 0.51."""
    want = _reference(True)
    _, hip = A._params(range(8))
    opt = _two_groups(hip, ema_decay=0.9, skip_nonfinite=True)
    for t in range(1, ema_ref.STEPS + 1):
        _set_hip_grads(t, hip, lambda k, t: ema_ref.recipe_grad(k, t, poison=True))
        before = (_ema_bits(hip, opt), _state_bits(hip, opt))
        opt.step()
        after = (_ema_bits(hip, opt), _state_bits(hip, opt))
        if t in ema_ref.POISON:
            assert _same(before[0], after[0]), 'step %d moved an average' % t
            assert all(_same(a, b) for a, b in zip(before[1], after[1])), 'step %d changed the state' % t
            assert float(opt.clip_record[2]) == 0.0
        else:
            assert float(opt.clip_record[2]) == 1.0
            assert all(b is None or not torch.equal(b, a) for k, (b, a) in enumerate(zip(before[0], after[0])) if k and ema_ref.has_grad(k, t)), t
        _cut_lr(t, opt)
    assert opt.grad_stats()['skipped'] == 2 == want['ref'].skipped
    worst = max(_fraction(opt.ema[p], want['ema'][(0.9, False)][30][k]) for k, p in enumerate(hip))
    print('guard: largest error / tolerance of the averages %.3g' % worst)
    assert worst <= 1.0
    A._compare('guard with the average', want['ps'], hip, want['ref'], opt)


# ------------------------------------------------------------------------------------------------ 5. swap
def _cbl_net(seed):
    from capsyolo_amd import models
    torch.manual_seed(seed)
    seq = collections.OrderedDict()
    models._cbl(seq, 1, 3, 64, 3, 1, 1)
    net = models.FusedBackbone(seq)
    with torch.no_grad():
        net.bn_1.running_mean.normal_(0.0, 0.1)
        net.bn_1.running_var.uniform_(0.5, 1.5)
        net.bn_1.weight.uniform_(0.5, 1.5)
        net.bn_1.bias.normal_(0.0, 0.1)
    return net.cuda()


def test_the_exchange_with_the_averaged_weights():
    """One conv -> BatchNorm -> LeakyReLU block (3 -> 64, 8 x 8, batch 2) in eval mode, so that the BatchNorm fold cache is in the way:
    inside ema_weights() the block computes what a fresh block loaded with ema_state_dict computes, not what it computes outside;
    after it, output and every parameter (address and bits) are what they were; step() inside is refused."""
    net = _cbl_net(5)
    params = list(net.parameters())
    opt = optim.Adam(params, lr=1e-2, ema_decay=0.5)
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g).cuda()
        opt.step()
    net.eval()
    x = torch.randn((2, 3, 8, 8), generator=g).cuda()
    sd = opt.ema_state_dict(net)
    assert list(sd) == [n for n, _ in net.named_parameters()] and all(not torch.equal(sd[n], p) for n, p in net.named_parameters())
    before = [(p.data_ptr(), _bits(p)) for p in params]
    with torch.no_grad():
        out_live = net(x).clone()                                        # (the fold cache now holds the live weights)
        with opt.ema_weights():
            out_avg = net(x).clone()
            assert all(torch.equal(p, sd[n]) for n, p in net.named_parameters())
            with pytest.raises(RuntimeError, match='ema_weights'):
                opt.step()
        out_back = net(x).clone()
    fresh = _cbl_net(6)
    fresh.load_state_dict(net.state_dict())
    missing = fresh.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all('running' in k or 'num_batches' in k for k in missing.missing_keys)
    fresh.eval()
    with torch.no_grad():
        out_fresh = fresh(x)
    assert torch.equal(out_avg, out_fresh)
    assert not torch.equal(out_avg, out_live) and float((out_avg - out_live).abs().max()) > 1e-3
    assert torch.equal(out_back, out_live)
    assert all(p.data_ptr() == a and torch.equal(_bits(p), b) for p, (a, b) in zip(params, before))
    assert all(torch.equal(opt.ema[p], sd[n]) for n, p in net.named_parameters())
    opt.graph_hyper = {}
    try:
        with pytest.raises(RuntimeError, match='captured step'):
            with opt.ema_weights():
                pass
    finally:
        opt.graph_hyper = None


# ------------------------------------------------------------------------------------------------ 6. checkpoint
class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


def test_checkpoint_round_trip(tmp_path):
    """ema_state_dict + optim_dict + the parameters through a file after 10 steps, into a fresh optimizer, 10 more steps: averages and
    parameters have the bits of 20 uninterrupted steps (warm-up schedule and the lagging parameter 2 included); torch.optim.Adam
    still loads the optim_dict."""
    idx = [0, 2, 5, 6]
    kw = dict(A.GROUPS[1], ema_decay=0.9, ema_warmup=True)

    def grads(t, hip):
        for p, k in zip(hip, idx):
            p.grad = _hand_over(k, A._grad(k, t)) if ema_ref.has_grad(k, t) else None
    _, straight = A._params(idx)
    o_straight = optim.Adam(straight, **kw)
    for t in range(1, 21):
        grads(t, straight)
        o_straight.step()
    _, first = A._params(idx)
    o_first = optim.Adam(first, **kw)
    for t in range(1, 11):
        grads(t, first)
        o_first.step()
    bag = _Bag(first)
    path = str(tmp_path / 'ckpt.pth.tar')
    torch.save({'state_dict': bag.state_dict(), 'optim_dict': o_first.state_dict(), 'ema_state_dict': o_first.ema_state_dict(bag)}, path)
    ck = torch.load(path, weights_only=False)
    assert sorted(ck['ema_state_dict']) == sorted(n for n, _ in bag.named_parameters()) == ['ps.%d' % i for i in range(4)]
    assert sorted(ck['optim_dict']) == ['param_groups', 'state']
    bag2 = _Bag([torch.nn.Parameter(torch.zeros(A.SHAPES[k], device='cuda')) for k in idx])
    bag2.load_state_dict(ck['state_dict'])
    second = list(bag2.ps)
    o_second = optim.Adam(second, lr=1.0, ema_decay=0.9, ema_warmup=True)
    o_second.load_state_dict(ck['optim_dict'])
    o_second.load_ema_state_dict(bag2, ck['ema_state_dict'])
    assert all(torch.equal(o_second.ema[a], o_first.ema[b]) and o_second.ema[a].data_ptr() != o_first.ema[b].data_ptr() for a, b in zip(second, first))
    for t in range(11, 21):
        grads(t, second)
        o_second.step()
    for k, (a, b) in enumerate(zip(second, straight)):
        assert torch.equal(_bits(a), _bits(b)), 'parameter %d' % k
        assert torch.equal(_bits(o_second.ema[a]), _bits(o_straight.ema[b])), 'average %d' % k
        assert int(o_second.state[a]['step']) == int(o_straight.state[b]['step']) == (20 if idx[k] != 2 else 13)
    cpu = [torch.nn.Parameter(p.detach().cpu().double()) for p in first]
    o_torch = torch.optim.Adam(cpu, lr=1.0)
    o_torch.load_state_dict(torch.load(path, weights_only=False, map_location='cpu')['optim_dict'])
    assert o_torch.param_groups[0]['lr'] == A.GROUPS[1]['lr'] and o_torch.state[cpu[0]]['exp_avg'].dtype == torch.float64
    assert torch.equal(o_torch.state[cpu[3]]['exp_avg'].float(), o_first.state[first[3]]['exp_avg'].cpu())


# ------------------------------------------------------------------------------------------------ 7. captured step
def test_graphed_step_keeps_the_average():
    """A CapsuleNet step on 8 synthetic samples (32 x 32, reconstruction on) with ema_decay = 0.9 and the warm-up, captured
    (cy_adam_step+dev+ema, eight scalars) and replayed 6 times against 6 eager steps from the same start.  The three warm-up steps of the
    capture are rolled back: every average equals its parameter afterwards.  The decay of replay t is (1 + t) / (10 + t): it can only
    have come from device memory (the capture froze every kernel argument), and hyper[6] holds 1 - 7/16 after the sixth.

    The averages are bit-identical to the eager run's (measured on the MI355X: largest difference of a parameter 0, of an average 0, the
    averages standing 7.1e-4 from the parameters).  That needs a CapsuleNet step that repeats to the bit: the bias gradients of the
    convolutions without BatchNorm (cy_channel_sum) used to be added with float atomics, which left two runs of these six steps 1e-6 to
    6e-5 apart in their parameters; they are summed in a fixed order now."""
    from capsyolo_amd import _lib, loss_fns, models
    from capsyolo_amd.graph_step import GraphedStep
    p = make_params(model='capsule', recon=True, device='cuda', batch_size=8)
    torch.manual_seed(3)
    net_e = models.CapsuleNet(p).cuda().train()
    net_g = models.CapsuleNet(p).cuda().train()
    net_g.load_state_dict(net_e.state_dict())
    xs = [torch.from_numpy(synth_images(8, 32, seed=200 + i)).cuda() for i in range(6)]
    ys = [torch.from_numpy(np.random.default_rng(400 + i).integers(0, 43, 8).astype(np.int64)).cuda() for i in range(6)]

    def fwd(m, x, y):
        s, rec = m(x, y, True)
        return s, loss_fns.capsule_loss(s, y, p, x, rec)
    pe, pg = [q for q in net_e.parameters() if q.requires_grad], [q for q in net_g.parameters() if q.requires_grad]
    opt_e = optim.Adam(pe, lr=1e-3, ema_decay=0.9, ema_warmup=True)
    opt_g = optim.Adam(pg, lr=1e-3, ema_decay=0.9, ema_warmup=True)
    _lib.TRACE = trace = []
    try:
        step = GraphedStep(net_g, fwd, opt_g, (xs[0], ys[0]), warmup=3)
        captured = [n for n in trace if n.startswith('cy_adam_step')]
        del trace[:]
        assert captured == ['cy_adam_step+ema'] * 3 + ['cy_adam_step+dev+ema']
        assert set(opt_g.ema) == set(pg) and all(torch.equal(opt_g.ema[q], q) and opt_g.ema[q].data_ptr() != q.data_ptr() for q in pg)
        for (n, a), (_, b) in zip(net_g.state_dict().items(), net_e.state_dict().items()):
            assert torch.equal(a, b), n
        for x, y in zip(xs, ys):
            _, l = fwd(net_e, x, y)
            opt_e.zero_grad()
            l.backward()
            opt_e.step()
            step(x, y)
        assert not any(n.startswith('cy_adam_step') and n != 'cy_adam_step+ema' for n in trace)       # the replays call nothing
        assert trace.count('cy_adam_step+ema') == 6
    finally:
        _lib.TRACE = None
    torch.cuda.synchronize()
    hyper = step._hyper_dev[id(opt_g.param_groups[0])].cpu()
    assert hyper.numel() == 8 and float(hyper[6]) == float(np.float32(1.0 - 7.0 / 16.0)) and float(hyper[7]) == 0.0
    assert int(opt_g.state[pg[0]]['step']) == int(opt_e.state[pe[0]]['step']) == 6
    diff_p = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pg, pe))
    diff_e = max(float((opt_g.ema[a] - opt_e.ema[b]).abs().max()) for a, b in zip(pg, pe))
    moved = max(float((opt_e.ema[b] - b.detach()).abs().max()) for b in pe)
    print('captured against eager after 6 steps: largest difference of a parameter %.3g, of an average %.3g (average - parameter: %.3g)'
          % (diff_p, diff_e, moved))
    assert moved > 0
    with opt_g.ema_weights():
        with pytest.raises(RuntimeError, match='ema_weights'):
            step(xs[0], ys[0])
    for k, (a, b) in enumerate(zip(pg, pe)):
        assert torch.equal(_bits(a), _bits(b)), 'parameter %d' % k
        assert torch.equal(_bits(opt_g.ema[a]), _bits(opt_e.ema[b])), 'average of parameter %d' % k


# ------------------------------------------------------------------------------------------------ 8. command line
def _main():
    spec = importlib.util.spec_from_file_location('cy_main', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_main_trains_saves_and_predicts_with_the_average(tmp_path, capsys):
    m = _main()
    with_ema, without = str(tmp_path / 'ema'), str(tmp_path / 'plain')
    for d in (with_ema, without):
        os.makedirs(d)
        json.dump(dict(batch_size=8, n_epochs=3, n_classes=43, lr_decay=0.1, capsule_input=32), open(os.path.join(d, 'params.json'), 'w'))
    m.main(['--model', 'capsule', '--synthetic', '64', '--n_epochs', '2', '--batch_size', '16', '--ema', '0.9', '--fix_ckpt_dir',
            '--model_dir', with_ema])
    ck = torch.load(os.path.join(with_ema, 'last.pth.tar'), weights_only=False, map_location='cpu')
    names = [n for n, _ in m.CapsuleNet(m.load_params(with_ema, m.parser.parse_args(['--model', 'capsule']))).named_parameters()]
    assert sorted(ck) == ['ema_state_dict', 'epoch', 'optim_dict', 'state_dict']
    assert list(ck['ema_state_dict']) == names and sorted(ck['optim_dict']) == ['param_groups', 'state']
    assert all(ck['ema_state_dict'][n].shape == ck['state_dict'][n].shape for n in names)
    assert any(not torch.equal(ck['ema_state_dict'][n], ck['state_dict'][n]) for n in names)
    assert os.path.exists(os.path.join(with_ema, 'best.pth.tar'))
    capsys.readouterr()
    predict = ['--model', 'capsule', '--mode', 'predict', '--restore', 'last', '--synthetic', '32']
    out_avg = m.main(predict + ['--use_ema', '--model_dir', with_ema])
    assert 'Using the averaged (EMA) parameters' in capsys.readouterr().out
    out_live = m.main(predict + ['--model_dir', with_ema])
    assert 'Using the averaged' not in capsys.readouterr().out
    assert set(out_avg) == set(out_live) == {'recog_pr', 'recog_acc', 'recog_auc'} and all(np.isfinite(float(v)) for v in out_avg.values())
    m.main(['--model', 'capsule', '--synthetic', '64', '--n_epochs', '1', '--batch_size', '16', '--fix_ckpt_dir', '--no_metric',
            '--model_dir', without])
    assert 'ema_state_dict' not in torch.load(os.path.join(without, 'last.pth.tar'), weights_only=False, map_location='cpu')
    with pytest.raises(SystemExit, match="has no 'ema_state_dict' entry: it was written by a training run without --ema"):
        m.main(predict + ['--use_ema', '--model_dir', without])

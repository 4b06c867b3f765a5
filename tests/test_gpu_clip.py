"""GPU tests of optim.Adam's gradient-norm clipping and non-finite guard: csrc/gradnorm.hip (cy_grad_sumsq_multi, cy_grad_clip_finish) and the
two Adam steps that read its record (cy_adam_step of csrc/adam.hip, host or device scalars), against tests/clip_ref.py (clip_grad_norm_ + torch.optim.Adam in float64 on the CPU; checked against the
written-out rule in tests/test_clip_host.py).  The recipe is clip_ref's: the 8 tensors of tests/test_gpu_adam.py, max_norm = 1.0, gradients that
clip on even steps and do not on odd ones.  Parameters, exp_avg and exp_avg_sq are held to test_gpu_adam.py's rule (rtol 1e-5, atol 1e-6).

Measured on the MI355X: the norm is within 1.5e-8 relative of float64 (bound 2^-23 = 1.2e-7); the largest error / tolerance of the
state comparisons is 0.58 (each test's docstring has its own)."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO, make_params, synth_images

from capsyolo_amd import optim

import clip_ref
import test_gpu_adam as A

pytestmark = pytest.mark.gpu

BIG = 256 * 16384 + 1                    # 257 chunks, the last of one element: with the 8 tensors, n_partial = 271 > the finish kernel's 256 threads


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def _state_bits(params, opt):
    out = []
    for p in params:
        st = opt.state.get(p) or {}
        out.append([_bits(p)] + [_bits(st[k]) for k in ('exp_avg', 'exp_avg_sq') if k in st])
    return out


def _same_bits(a, b):
    return all(len(x) == len(y) and all(torch.equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


def _hand_over(k, g):
    """The gradient on the device as test_gpu_adam hands it over: tensor 6 (32768 elements) as a non-contiguous transpose."""
    if k == 6:
        gt = g.t().contiguous().cuda().t()
        assert not gt.is_contiguous()
        return gt
    return g.cuda()


def _set_recipe_grads(t, ref, hip, skip=True, poison=None):
    for k, (pr, ph) in enumerate(zip(ref, hip)):
        if skip and not clip_ref.has_grad(k, t):
            pr.grad, ph.grad = None, None
            continue
        g = clip_ref.recipe_grad(k, t).clone()
        if poison and t in poison and poison[t][0] == k:
            g.view(-1)[poison[t][1]] = poison[t][2]
        pr.grad, ph.grad = g.double(), _hand_over(k, g)


def _two_groups(max_norm, guard):
    ref, hip = A._params(range(8))
    o_ref = clip_ref.ClipRef([dict(params=ref[:4], **A.GROUPS[0]), dict(params=ref[4:], **A.GROUPS[1])], max_norm, guard)
    o_hip = optim.Adam([dict(params=hip[:4], **A.GROUPS[0]), dict(params=hip[4:], **A.GROUPS[1])], max_grad_norm=max_norm, skip_nonfinite=guard)
    return ref, hip, o_ref, o_hip


def _norm64(grads):
    return float(np.sqrt(sum(float((g.detach().cpu().double() ** 2).sum()) for g in grads)))


@pytest.mark.parametrize('layout', ['tensors', 'bucket_views'])
def test_norm_against_float64(layout):
    """record[0] of one step against the float64 norm of the same fp32 gradients, within 2^-23 relative (the double sums contribute about
    n 2^-53, which leaves the one rounding to fp32), and a second run on the same gradients gives the same bits.  'tensors': the 8 sizes
    (32768 as a non-contiguous transpose) and one tensor of 256 * 16384 + 1 elements; 'bucket_views': the 8 sizes as views at odd element
    offsets of one flat buffer, as dp.GradBucket leaves them."""
    sizes = A.SIZES + ([BIG] if layout == 'tensors' else [])
    rng = np.random.default_rng(77)
    params = [torch.nn.Parameter(torch.zeros(A.SHAPES[k] if k < 8 else (n,), device='cuda')) for k, n in enumerate(sizes)]
    if layout == 'tensors':
        for k, p in enumerate(params):
            g = torch.from_numpy((rng.standard_normal(sizes[k]) * 10.0 ** ((k % 4) - 2)).astype(np.float32)).reshape(p.shape)
            p.grad = _hand_over(k, g)
    else:
        flat = torch.from_numpy(rng.standard_normal(sum(sizes) + 1).astype(np.float32)).cuda()
        off = 1
        for k, p in enumerate(params):
            p.grad = flat[off:off + sizes[k]].view(p.shape)
            assert (p.grad.data_ptr() - flat.data_ptr()) // 4 == off and p.grad.is_contiguous()
            off += sizes[k]
        assert any((p.grad.data_ptr() // 4) % 4 for p in params)            # not 16-byte aligned
    want = _norm64([p.grad for p in params])
    opt = optim.Adam(params, lr=1e-3, max_grad_norm=1.0)
    grads = [_bits(p.grad) for p in params]
    opt.step()
    first = _bits(opt.clip_record)
    stats = opt.grad_stats()
    opt.step()
    second = _bits(opt.clip_record)
    print('%s: norm %.9g, float64 %.17g, relative error %.3g (bound %.3g)' % (layout, stats['norm'], want, abs(stats['norm'] - want) / want, 2.0 ** -23))
    assert abs(stats['norm'] - want) <= 2.0 ** -23 * want
    assert stats['coef'] == float(np.float32(1.0 / (want + 1e-6))) or abs(stats['coef'] * (want + 1e-6) - 1.0) <= 2.0 ** -22
    assert stats['skipped'] == 0 and float(opt.clip_record[2]) == 1.0
    assert torch.equal(first, second)
    assert all(torch.equal(a, _bits(p.grad)) for a, p in zip(grads, params))


def test_clipped_steps_two_groups():
    """10 steps of the recipe through cy_adam_step+clip: two groups (ONE norm over both, three Adam launches in the steps where parameter
    2 lags), even steps clipped.  p.grad keeps its bits.  Measured on the MI355X: largest error / tolerance 0.56 on the parameters (the fp32
    1 - beta2 of DESIGN.md section 6n, as in test_gpu_adam.py), 8e-4 on exp_avg, 1e-5 on exp_avg_sq."""
    ref, hip, o_ref, o_hip = _two_groups(clip_ref.MAX_NORM, False)
    coefs = []
    for t in range(1, 11):
        _set_recipe_grads(t, ref, hip)
        grads = [None if p.grad is None else _bits(p.grad) for p in hip]
        o_ref.step()
        o_hip.step()
        assert all(p.grad is None or torch.equal(g, _bits(p.grad)) for g, p in zip(grads, hip))
        s = o_hip.grad_stats()
        assert abs(s['norm'] - o_ref.norm) <= 2.0 ** -23 * o_ref.norm and abs(s['coef'] - o_ref.coef) <= 2.0 ** -23 * o_ref.coef, t
        coefs.append(s['coef'])
    assert all(c == 1.0 for c in coefs[0::2]) and all(c < 0.1 for c in coefs[1::2]), coefs
    assert int(o_hip.state[hip[2]]['step']) == 6 and int(o_hip.state[hip[0]]['step']) == 10
    A._compare('clipped, two groups', ref, hip, o_ref, o_hip)


@pytest.mark.parametrize('gi', [0, 1])
def test_clipped_steps_device_scalar_kernel(gi):
    """The same through cy_adam_step+dev+clip, launched eagerly with the tables and scalars of graph_step.GraphedStep as
    test_gpu_adam.test_device_scalar_kernel_without_a_capture does (one group, a gradient for every parameter: the captured path
    refuses anything else).  Measured on the MI355X: largest error / tolerance 0.58 / 7e-4 / 6e-6 (parameters / exp_avg /
    exp_avg_sq) with the default betas, 0.04 / 6e-4 / 8e-6 with betas (0.5, 0.9)."""
    ref, hip = A._params(range(8))
    o_ref = clip_ref.ClipRef([dict(params=ref, **A.GROUPS[gi])], clip_ref.MAX_NORM, False)
    o_hip = optim.Adam(hip, max_grad_norm=clip_ref.MAX_NORM, **A.GROUPS[gi])
    group = o_hip.param_groups[0]
    hyper = torch.zeros(6, dtype=torch.float32, device='cuda')
    tables = (torch.empty((8, 5), dtype=torch.int64).pin_memory(), torch.empty((8, 5), dtype=torch.int64, device='cuda'))
    coefs = []
    try:
        for t in range(1, 11):
            _set_recipe_grads(t, ref, hip, skip=False)
            o_ref.step()
            if t == 2:                                                   # after one eager step (it built the block map)
                o_hip.graph_hyper, o_hip.graph_tables = {id(group): hyper}, {id(group): tables}
            if t >= 2:
                hyper.copy_(torch.tensor(o_hip.step_scalars(group, t), dtype=torch.float32))
            o_hip.step()
            torch.cuda.synchronize()
            coefs.append(o_hip.grad_stats()['coef'])
    finally:
        o_hip.graph_hyper, o_hip.graph_tables = None, None
    assert all(c == 1.0 for c in coefs[0::2]) and all(c < 0.1 for c in coefs[1::2]), coefs
    A._compare('clipped, device scalars, group %d' % gi, ref, hip, o_ref, o_hip)


@pytest.mark.parametrize('kernel', ['cy_adam_step+clip', 'cy_adam_step+dev+clip'])
def test_inactive_clipping_is_the_plain_step(kernel):
    """max_grad_norm = 1e30 never clips (coef is exactly 1.0f): parameters, exp_avg and exp_avg_sq of 5 steps have the bits of an Adam without
    the option, for both kernels."""
    from capsyolo_amd import _lib
    dev = kernel.endswith('dev+clip')
    _, plain = A._params(range(8))
    _, clip = A._params(range(8))
    o_plain, o_clip = optim.Adam(plain, **A.GROUPS[1]), optim.Adam(clip, max_grad_norm=1e30, **A.GROUPS[1])
    hyper = torch.zeros(6, dtype=torch.float32, device='cuda')
    _lib.TRACE = trace = []
    try:
        for t in range(1, 6):
            for k in range(8):
                g = A._grad(k, t)
                plain[k].grad, clip[k].grad = _hand_over(k, g), _hand_over(k, g)
            if dev and t == 2:
                for o in (o_plain, o_clip):
                    group = o.param_groups[0]
                    o.graph_hyper = {id(group): hyper}
                    o.graph_tables = {id(group): (torch.empty((8, 5), dtype=torch.int64).pin_memory(), torch.empty((8, 5), dtype=torch.int64, device='cuda'))}
            if dev and t >= 2:
                hyper.copy_(torch.tensor(o_plain.step_scalars(o_plain.param_groups[0], t), dtype=torch.float32))
            o_plain.step()
            torch.cuda.synchronize()
            o_clip.step()
            torch.cuda.synchronize()
    finally:
        _lib.TRACE = None
        for o in (o_plain, o_clip):
            o.graph_hyper, o.graph_tables = None, None
    assert trace.count(kernel) == (4 if dev else 5) and trace.count('cy_grad_clip_finish') == 5, trace
    assert o_plain._clip_buf is None and o_plain._partial is None        # with the options off none of the device state exists
    assert o_clip.grad_stats()['coef'] == 1.0
    assert _same_bits(_state_bits(plain, o_plain), _state_bits(clip, o_clip))


POISON = {3: (0, 0, float('inf')),               # +inf in the 1-element tensor
          5: (7, 70000, float('nan')),           # NaN in the last element of the 70001 tensor (its tail chunk)
          6: (6, 16384, float('-inf'))}          # -inf at element 16384 of the 32768 tensor (the first element of a chunk)


@pytest.mark.parametrize('max_norm', [None, clip_ref.MAX_NORM])
def test_guard_skips_the_poisoned_steps(max_norm):
    """skip_nonfinite over 8 steps of the recipe with three poisoned steps: around each, every parameter, exp_avg and exp_avg_sq keeps its
    bits; skipped counts 3; the host's step counts advance all the same, and the final state is clip_ref's.  Guard only, and guard with
    clipping.  Measured on the MI355X: largest error / tolerance 0.28 / 0.010 / 0.005 (parameters / exp_avg /
    exp_avg_sq) guard only, 0.28 / 6e-4 / 9e-6 with clipping."""
    ref, hip, o_ref, o_hip = _two_groups(max_norm, True)
    for t in range(1, 9):
        _set_recipe_grads(t, ref, hip, poison=POISON)
        before = _state_bits(hip, o_hip)
        o_ref.step()
        o_hip.step()
        after = _state_bits(hip, o_hip)
        if t in POISON:
            assert _same_bits(before, after), 'step %d changed something' % t
            assert float(o_hip.clip_record[2]) == 0.0 and not np.isfinite(o_hip.grad_stats()['norm'])
        else:
            assert not _same_bits(before, after) and float(o_hip.clip_record[2]) == 1.0
    assert o_hip.grad_stats()['skipped'] == 3 == o_ref.skipped
    assert int(o_hip.state[hip[0]]['step']) == 8 and int(o_hip.state[hip[2]]['step']) == 5
    A._compare('guard, max_norm %s' % max_norm, ref, hip, o_ref, o_hip)


def test_a_step_without_gradients_launches_nothing():
    from capsyolo_amd import _lib
    p = torch.nn.Parameter(torch.zeros(5, device='cuda'))
    o = optim.Adam([p], lr=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
    _lib.TRACE = trace = []
    try:
        o.step()
    finally:
        _lib.TRACE = None
    assert trace == [] and o.clip_record is None


def test_graphed_step_clips_and_skips():
    """The CapsuleNet step of test_gpu_models.test_graphed_step_equals_eager_steps (batch 16, 32 x 32, 6 batches) with max_grad_norm = 0.5 and
    skip_nonfinite, captured and replayed against the same steps run eagerly; batch 3 has one NaN pixel (CapsuleNet has no BatchNorm: a bad
    batch leaves no trace outside the optimizer).  The capture is made ON the NaN batch, so its three warm-up steps are skipped steps:
    skipped must still read 0 after the construction."""
    from capsyolo_amd import loss_fns, models
    from capsyolo_amd.graph_step import GraphedStep
    p = make_params(model='capsule', recon=True, device='cuda', batch_size=16)
    torch.manual_seed(3)
    net_e = models.CapsuleNet(p).cuda().train()
    net_g = models.CapsuleNet(p).cuda().train()
    net_g.load_state_dict(net_e.state_dict())
    xs = [torch.from_numpy(synth_images(16, 32, seed=200 + i)).cuda() for i in range(6)]
    ys = [torch.from_numpy(np.random.default_rng(400 + i).integers(0, 43, 16).astype(np.int64)).cuda() for i in range(6)]
    xs[3][5, 1, 7, 9] = float('nan')

    def fwd(m, x, y):
        s, rec = m(x, y, True)
        return s, loss_fns.capsule_loss(s, y, p, x, rec)
    pe, pg = [q for q in net_e.parameters() if q.requires_grad], [q for q in net_g.parameters() if q.requires_grad]
    opt_e = optim.Adam(pe, lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
    opt_g = optim.Adam(pg, lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
    step = GraphedStep(net_g, fwd, opt_g, (xs[3], ys[3]), warmup=3)
    assert opt_g.grad_stats()['skipped'] == 0
    for (n, a), (_, b) in zip(net_g.state_dict().items(), net_e.state_dict().items()):
        assert torch.equal(a, b), n
    le, lg, norms = [], [], []
    for i, (x, y) in enumerate(zip(xs, ys)):
        _, l = fwd(net_e, x, y)
        opt_e.zero_grad()
        l.backward()
        opt_e.step()
        le.append(l.item())
        before = _state_bits(pg, opt_g)
        lg.append(step(x, y)[1].item())
        after = _state_bits(pg, opt_g)
        assert _same_bits(before, after) == (i == 3), i
        norms.append((opt_e.grad_stats()['norm'], opt_g.grad_stats()['norm']))
    print('eager  ', ' '.join('%.6f' % v for v in le))
    print('graphed', ' '.join('%.6f' % v for v in lg))
    print('norms  ', norms)
    assert not np.isfinite(le[3]) and not np.isfinite(lg[3])
    keep = [i for i in range(6) if i != 3]
    assert np.all(np.isfinite([le[i] for i in keep]))
    np.testing.assert_allclose([lg[i] for i in keep], [le[i] for i in keep], rtol=2e-5, atol=1e-6)
    for (n, a), (_, b) in zip(net_g.named_parameters(), net_e.named_parameters()):
        assert torch.isfinite(a).all() and float((a.detach() - b.detach()).abs().max()) <= 2e-4, n
    assert opt_e.grad_stats()['skipped'] == 1 and opt_g.grad_stats()['skipped'] == 1
    assert int(opt_g.state[pg[0]]['step']) == int(opt_e.state[pe[0]]['step']) == 6
    opt_g.max_grad_norm = 0.25                            # a frozen kernel argument of the capture
    with pytest.raises(RuntimeError, match='frozen'):
        step(xs[0], ys[0])


@pytest.mark.parametrize('graph', [False, True])
def test_main_reports_norm_and_skipped(tmp_path, capsys, graph):
    spec = importlib.util.spec_from_file_location('cy_main', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    mdir = str(tmp_path / 'caps')
    os.makedirs(mdir)
    json.dump(dict(batch_size=8, n_epochs=3, n_classes=43, lr_decay=0.1, capsule_input=32), open(os.path.join(mdir, 'params.json'), 'w'))
    losses_tr, losses_ev = m.main(['--model', 'capsule', '--mode', 'train', '--synthetic', '32', '--n_epochs', '1', '--batch_size', '16',
                                   '--clip_norm', '0.5', '--skip_nonfinite', '--no_metric', '--model_dir', mdir, '--fix_ckpt_dir']
                                  + (['--graph'] if graph else []))
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith('epoch 1 ')]
    assert len(line) == 1, out
    found = re.search(r'\| grad norm: (\S+) \| skipped (\d+)$', line[0])
    assert found, line[0]
    assert np.isfinite(float(found.group(1))) and float(found.group(1)) > 0 and int(found.group(2)) == 0
    assert len(losses_tr) == 1 and np.isfinite(losses_tr[0]) and np.isfinite(losses_ev[0])

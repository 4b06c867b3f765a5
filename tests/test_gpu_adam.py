"""GPU tests of csrc/adam.hip behind capsyolo_amd.optim.Adam: both kernels (cy_adam_step, and cy_adam_step+dev with its scalars
in device memory, otherwise reached through a captured graph only) against torch.optim.Adam on float64 CPU copies, over tensor
sizes around the 16384-element chunk, two parameter groups, hyper-parameters other than the defaults, a learning rate that changes,
gradients with exact zeros and a parameter that has no gradient in some steps; and optimizer checkpoints in both directions.
The tolerance is that of test_adam_matches_torch (rtol 1e-5, atol 1e-6); torch's own fp32 run of the recipe stays within a tenth of
it against fp64.

Measured on the MI355X (largest error / tolerance): with the default betas 0.60 on the parameters and 0.55 on exp_avg_sq (both kernels),
with betas (0.5, 0.9) 0.07 and 0.04.  The first pair is a finding, not rounding noise: the kernels form 1 - beta2 in fp32 from the
rounded beta2, and 1.f - 0.999f is 1.29e-5 (relative) below 0.001; torch rounds 1 - beta2 once, from double."""
import io

import numpy as np
import pytest
import torch

from capsyolo_amd import optim

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 257, 16383, 16384, 16385, 32768, 70001]
SHAPES = [(n,) for n in SIZES]
SHAPES[6] = (128, 256)                  # 32768 elements; its gradient is handed over as the transpose of a (256, 128) tensor
GROUPS = [dict(lr=1e-2), dict(lr=3e-3, betas=(0.5, 0.9), eps=1e-3)]
STEPS, RTOL, ATOL = 30, 1e-5, 1e-6


def _init(k):
    return torch.from_numpy(np.random.default_rng(1000 + k).standard_normal(SHAPES[k]).astype(np.float32))


def _grad(k, t):
    """fp32 gradient of parameter k in step t (1-based): normal x 10^((k % 4) - 3), every seventh element exactly 0."""
    g = np.random.default_rng(10000 * t + k).standard_normal(SIZES[k]) * 10.0 ** ((k % 4) - 3)
    g[::7] = 0.0
    return torch.from_numpy(g.astype(np.float32).reshape(SHAPES[k]))


def _set_grads(t, ref, hip, skip=True):
    for k, (pr, ph) in enumerate(zip(ref, hip)):
        if skip and k == 2 and t % 3 == 1:                              # parameter 2 has no gradient in steps 1, 4, 7, ...
            pr.grad, ph.grad = None, None
            continue
        g = _grad(k, t)
        pr.grad = g.double()
        if k == 6:
            gt = g.t().contiguous().cuda().t()
            assert not gt.is_contiguous()
            ph.grad = gt
        else:
            ph.grad = g.cuda()


def _fraction(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    return float(((got - want).abs() / (ATOL + RTOL * want.abs())).max())


def _compare(tag, ref, hip, o_ref, o_hip):
    worst = {}
    for k, (pr, ph) in enumerate(zip(ref, hip)):
        sr, sh = o_ref.state[pr], o_hip.state[ph]
        assert int(sh['step']) == int(sr['step']), 'step count of parameter %d' % k
        for what, a, b in (('param', ph, pr), ('exp_avg', sh['exp_avg'], sr['exp_avg']), ('exp_avg_sq', sh['exp_avg_sq'], sr['exp_avg_sq'])):
            worst[what] = max(worst.get(what, 0.0), _fraction(a, b))
    print('%s: largest error / tolerance %s' % (tag, dict((k, '%.3g' % v) for k, v in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    return worst


def _through_a_file(state_dict):
    """The state_dict as a checkpoint hands it over (torch.save, torch.load): load_state_dict keeps the 'step' tensors it is given, and two
    live optimizers must not share them."""
    buf = io.BytesIO()
    torch.save(state_dict, buf)
    buf.seek(0)
    return torch.load(buf)


def _params(indices):
    ref = [torch.nn.Parameter(_init(k).double()) for k in indices]
    hip = [torch.nn.Parameter(_init(k).cuda()) for k in indices]
    return ref, hip


def test_two_groups_thirty_steps():
    ref, hip = _params(range(8))
    o_ref = torch.optim.Adam([dict(params=ref[:4], **GROUPS[0]), dict(params=ref[4:], **GROUPS[1])])
    o_hip = optim.Adam([dict(params=hip[:4], **GROUPS[0]), dict(params=hip[4:], **GROUPS[1])])
    for t in range(1, STEPS + 1):
        _set_grads(t, ref, hip)
        o_ref.step()
        o_hip.step()
        if t == 10:
            _compare('step 10', ref, hip, o_ref, o_hip)
            for o in (o_ref, o_hip):
                for g in o.param_groups:
                    g['lr'] *= 0.1
    assert int(o_hip.state[hip[2]]['step']) == 20 and int(o_hip.state[hip[0]]['step']) == 30
    _compare('step 30', ref, hip, o_ref, o_hip)
    zero = _grad(7, 1).reshape(-1) == 0
    assert int(zero.sum()) == 10001                                      # the exact zeros are there


@pytest.mark.parametrize('gi', [0, 1])
def test_device_scalar_kernel_without_a_capture(gi):
    """cy_adam_step+dev with the tables and scalars that graph_step.GraphedStep gives it, launched eagerly.  One group and a gradient
    for every parameter in every step: a captured step has one block map and a fixed set of parameters by design (optim.Adam refuses
    anything else on this path).  The device is synchronised after every step because this test rewrites the ONE pinned table per
    step that a capture reads once."""
    ref, hip = _params(range(8))
    o_ref, o_hip = torch.optim.Adam(ref, **GROUPS[gi]), optim.Adam(hip, **GROUPS[gi])
    group = o_hip.param_groups[0]
    hyper = torch.zeros(6, dtype=torch.float32, device='cuda')
    tables = (torch.empty((8, 5), dtype=torch.int64).pin_memory(), torch.empty((8, 5), dtype=torch.int64, device='cuda'))
    try:
        for t in range(1, STEPS + 1):
            _set_grads(t, ref, hip, skip=False)
            o_ref.step()
            if t == 2:                                                   # after one eager step (it built the block map)
                o_hip.graph_hyper, o_hip.graph_tables = {id(group): hyper}, {id(group): tables}
            if t >= 2:
                hyper.copy_(torch.tensor(o_hip.step_scalars(group, t), dtype=torch.float32))
            o_hip.step()
            torch.cuda.synchronize()
            if t == 10:
                for o in (o_ref, o_hip):
                    o.param_groups[0]['lr'] *= 0.1
    finally:
        o_hip.graph_hyper, o_hip.graph_tables = None, None
    _compare('device scalars, group %d' % gi, ref, hip, o_ref, o_hip)


def test_captured_path_refuses_a_lagging_parameter():
    ref, hip = _params([0, 1, 2])
    o_hip = optim.Adam(hip, lr=1e-2)
    for k, p in enumerate(hip[:2]):
        p.grad = _grad(k, 1).cuda()
    o_hip.step()
    for k, p in enumerate(hip):
        p.grad = _grad(k, 2).cuda()
    o_hip.graph_hyper = {}
    try:
        with pytest.raises(RuntimeError, match='share their step count'):
            o_hip.step()
    finally:
        o_hip.graph_hyper = None


@pytest.mark.parametrize('direction', ['torch_to_hip', 'hip_to_torch'])
def test_checkpoint_interchange(direction):
    """A state_dict of one optimizer after five steps, loaded into the other, continues to the parameters torch reaches on its own."""
    idx = [0, 2, 5, 6]
    ref, hip = _params(idx)
    hp = GROUPS[1]
    o_ref, o_hip = torch.optim.Adam(ref, **hp), optim.Adam(hip, **hp)

    def grads(t):
        for pr, ph, k in zip(ref, hip, idx):
            g = _grad(k, t)
            pr.grad, ph.grad = g.double(), g.cuda()
    for t in range(1, 6):
        grads(t)
        o_ref.step()
        o_hip.step()
    _compare('before the hand-over', ref, hip, o_ref, o_hip)
    if direction == 'torch_to_hip':
        hip2 = [torch.nn.Parameter(p.detach().float().cuda()) for p in ref]
        o2 = optim.Adam(hip2, lr=1.0)                                    # the loaded group brings its own hyper-parameters
        o2.load_state_dict(_through_a_file(o_ref.state_dict()))
        assert o2.param_groups[0]['lr'] == hp['lr'] and tuple(o2.param_groups[0]['betas']) == hp['betas']
        ref2, o_ref2 = ref, o_ref
    else:
        ref2 = [torch.nn.Parameter(p.detach().cpu().double()) for p in hip]
        o_ref2 = torch.optim.Adam(ref2, lr=1.0)
        o_ref2.load_state_dict(_through_a_file(o_hip.state_dict()))
        assert o_ref2.param_groups[0]['lr'] == hp['lr'] and o_ref2.state[ref2[0]]['exp_avg'].dtype == torch.float64
        hip2, o2 = hip, o_hip
    for t in range(6, 11):
        for pr, ph, k in zip(ref2, hip2, idx):
            g = _grad(k, t)
            pr.grad, ph.grad = g.double(), g.cuda()
        o_ref2.step()
        o2.step()
    _compare(direction, ref2, hip2, o_ref2, o2)


def test_other_flavours_of_adam_are_refused():
    p = torch.nn.Parameter(torch.zeros(4, device='cuda'))
    p.grad = torch.ones(4, device='cuda')
    o = optim.Adam([p], lr=1e-2)
    o.param_groups[0]['weight_decay'] = 0.1                              # as a checkpoint of torch.optim.Adam may bring it
    with pytest.raises(RuntimeError, match='weight_decay'):
        o.step()
    assert not p.detach().cpu().numpy().any()

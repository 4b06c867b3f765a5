"""GPU tests of csrc/linear.hip: the split-K forward, the input and weight gradients, their autograd wrapper and the softmax
cross-entropy.  Two yardsticks: integer inputs, on which every summation order gives the same fp32 number (exact equality with
int64 numpy), and fp64 numpy on standard-normal inputs, where a kernel may be 20 x as far from fp64 as torch's CPU fp32 product of
the same inputs is (the rule of tests/test_gpu_models.py), with a floor of 1e-6."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from capsyolo_amd import _lib, ops

pytestmark = pytest.mark.gpu

# one row; rows past a 16-row tile; rows past 128; N past 128 with an edge and a K that is no multiple of a slice (3 shares of 192);
# many shares at one and at a quarter of a row tile
SHAPES = [(1, 43, 128), (17, 43, 128), (130, 43, 128), (33, 130, 516), (16, 128, 32768), (4, 128, 32768)]
LONG = [(16, 128, 32768), (4, 128, 32768)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def k_fwd(x, w, b, act):
    (M, K), N = x.shape, w.shape[0]
    y = _nan(M, N)
    nws = _lib.query('cy_linear_fwd_ws_floats', M, N, K)
    ws = _nan(max(nws, 1))
    _lib.call('cy_linear_fwd', x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(), M, N, K, act,
              ws.data_ptr() if nws else None, _st())
    return y


def k_dgrad(dy, w, x_mask):
    (M, N), K = dy.shape, w.shape[1]
    dx = _nan(M, K)
    _lib.call('cy_linear_dgrad', dy.data_ptr(), w.data_ptr(), dx.data_ptr(), None if x_mask is None else x_mask.data_ptr(), M, N, K, _st())
    return dx


def k_wgrad(dy, x, with_db=True):
    (M, N), K = dy.shape, x.shape[1]
    dw, db = _nan(N, K), _nan(N)
    _lib.call('cy_linear_wgrad', dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr() if with_db else None, M, N, K, _st())
    return dw, db


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rel_l2(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d, n = np.linalg.norm((a - ref).ravel()), np.linalg.norm(ref.ravel())
    return d / n if n > 0 else d


def within_rule(name, got, cpu32, ref64):
    e_hip, e_32 = rel_l2(got, ref64), rel_l2(cpu32, ref64)
    print('%s: HIP %.3e, torch CPU fp32 %.3e (relative L2 against fp64)' % (name, e_hip, e_32))
    assert np.isfinite(e_hip) and e_hip <= max(1e-6, 20 * e_32), '%s: HIP %.3e vs CPU fp32 %.3e' % (name, e_hip, e_32)
    return e_hip, e_32


@functools.lru_cache(maxsize=None)
def int_case(M, N, K):
    """Integer inputs in -2 .. 2 and the int64 results (computed once per shape, never written)."""
    rng = np.random.default_rng(1000 + M + 7 * N + K)
    x, w, dy = (rng.integers(-2, 3, s).astype(np.int64) for s in ((M, K), (N, K), (M, N)))
    b = rng.integers(-2, 3, (N,)).astype(np.int64)
    z = x @ w.T
    return dict(x=x, w=w, dy=dy, b=b, z=z, dx=dy @ w, dw=dy.T @ x, db=dy.sum(0))


@functools.lru_cache(maxsize=None)
def normal_case(M, N, K):
    rng = np.random.default_rng(2000 + M + 7 * N + K)
    x, w, dy = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), (M, N)))
    b = rng.standard_normal((N,)).astype(np.float32)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    tx, tw, tdy, tb = (torch.from_numpy(a) for a in (x, w, dy, b))
    return dict(x=x, w=w, dy=dy, b=b,
                y64=x64 @ w64.T + b, dx64=dy64 @ w64, dw64=dy64.T @ x64, db64=dy64.sum(0),
                y32=F.linear(tx, tw, tb).numpy(), dx32=(tdy @ tw).numpy(), dw32=(tdy.t() @ tx).numpy(), db32=tdy.sum(0).numpy())


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_exact_on_integers(M, N, K):
    c = int_case(M, N, K)
    assert max(np.abs(c[k]).max() for k in ('z', 'dx', 'dw', 'db')) + 2 < 2 ** 24     # every partial sum is an exact fp32 integer
    x, w, dy, b = _dev(c['x']), _dev(c['w']), _dev(c['dy']), _dev(c['b'])
    shares = _lib.query('cy_linear_fwd_shares', M, N, K)
    print('(%d,%d,%d): %d shares of %d' % (M, N, K, shares, _lib.query('cy_linear_fwd_slice', M, N, K)))
    assert (shares == 1) == (K == 128) and (K != 516 or shares == 3)
    for bias in (None, b):
        for act in (0, 1):
            want = c['z'] + (0 if bias is None else c['b'])
            want = np.maximum(want, 0) if act else want
            np.testing.assert_array_equal(k_fwd(x, w, bias, act).cpu().numpy(), want.astype(np.float32), err_msg='forward bias=%s act=%d' % (bias is not None, act))
    np.testing.assert_array_equal(k_dgrad(dy, w, None).cpu().numpy(), c['dx'].astype(np.float32))
    np.testing.assert_array_equal(k_dgrad(dy, w, x).cpu().numpy(), np.where(c['x'] > 0, c['dx'], 0).astype(np.float32))
    dw, db = k_wgrad(dy, x)
    np.testing.assert_array_equal(dw.cpu().numpy(), c['dw'].astype(np.float32))
    np.testing.assert_array_equal(db.cpu().numpy(), c['db'].astype(np.float32))
    dw2, db2 = k_wgrad(dy, x, with_db=False)                             # db is optional: dW alone, db untouched
    np.testing.assert_array_equal(dw2.cpu().numpy(), c['dw'].astype(np.float32))
    assert torch.isnan(db2).all()


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_against_fp64(M, N, K):
    c = normal_case(M, N, K)
    x, w, dy, b = _dev(c['x']), _dev(c['w']), _dev(c['dy']), _dev(c['b'])
    within_rule('forward', k_fwd(x, w, b, 0).cpu().numpy(), c['y32'], c['y64'])
    within_rule('forward+relu', k_fwd(x, w, b, 1).cpu().numpy(), np.maximum(c['y32'], 0), np.maximum(c['y64'], 0))
    within_rule('dgrad', k_dgrad(dy, w, None).cpu().numpy(), c['dx32'], c['dx64'])
    within_rule('dgrad masked', k_dgrad(dy, w, x).cpu().numpy(), np.where(c['x'] > 0, c['dx32'], 0), np.where(c['x'] > 0, c['dx64'], 0))
    dw, db = k_wgrad(dy, x)
    within_rule('wgrad', dw.cpu().numpy(), c['dw32'], c['dw64'])
    within_rule('db', db.cpu().numpy(), c['db32'], c['db64'])


@pytest.mark.parametrize('M,N,K', LONG)
def test_two_runs_identical_bits(M, N, K):
    c = normal_case(M, N, K)
    x, w, dy, b = _dev(c['x']), _dev(c['w']), _dev(c['dy']), _dev(c['b'])
    for name, run in (('forward', lambda: k_fwd(x, w, b, 1)), ('dgrad', lambda: k_dgrad(dy, w, x)),
                      ('wgrad', lambda: torch.cat([t.reshape(-1) for t in k_wgrad(dy, x)]))):
        a, again = run(), run()
        assert not torch.isnan(a).any() and torch.equal(a.view(torch.int32), again.view(torch.int32)), name


# ------------------------------------------------------------------------------------------------ autograd
@functools.lru_cache(maxsize=None)
def mlp_case():
    """x [17,516] -> Linear(516,128) -> ReLU -> Linear(128,43), cotangent g: gradients in fp64 and in fp32 on the CPU."""
    rng = np.random.default_rng(31)
    arrs = dict(x=rng.standard_normal((17, 516)), w1=rng.standard_normal((128, 516)) / 16, b1=rng.standard_normal(128),
                w2=rng.standard_normal((43, 128)) / 8, b2=rng.standard_normal(43), g=rng.standard_normal((17, 43)))
    arrs = dict((k, v.astype(np.float32)) for k, v in arrs.items())
    out = dict(arrs=arrs)
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        t = dict((k, torch.from_numpy(v).to(dt).requires_grad_(k != 'g')) for k, v in arrs.items())
        z = F.linear(t['x'], t['w1'], t['b1'])
        y = F.linear(torch.relu(z), t['w2'], t['b2'])
        (y * t['g']).sum().backward()
        out[tag] = dict((k, t[k].grad.numpy()) for k in ('x', 'w1', 'b1', 'w2', 'b2'))
        out[tag]['y'] = y.detach().numpy()
        h = torch.relu(F.linear(t['x'], t['w1'], t['b1']))
        (gh,) = torch.autograd.grad((h * t['g'][:, :1]).sum(), t['x'])
        out[tag]['x_alone'] = gh.numpy()
        if tag == '64':
            assert float(z.detach().abs().min()) > 1e-4       # no pre-activation so close to 0 that fp32 could flip its mask
    return out


def test_autograd_chain():
    c = mlp_case()
    t = dict((k, _dev(v).requires_grad_(k != 'g')) for k, v in c['arrs'].items())
    _lib.TRACE = trace = []
    try:
        h = ops.linear(t['x'], t['w1'], t['b1'], relu=True)
        y = ops.linear(h, t['w2'], t['b2'])
        (y * t['g']).sum().backward()
    finally:
        _lib.TRACE = None
    assert trace.count('cy_linear_fwd') == 2 and trace.count('cy_linear_dgrad') == 2 and trace.count('cy_linear_wgrad') == 2
    assert 'cy_act_bwd' not in trace                          # the ReLU's backward ran in the second layer's dgrad store
    assert (h.detach() >= 0).all() and (h.detach() == 0).any()
    within_rule('y', y.detach().cpu().numpy(), c['32']['y'], c['64']['y'])
    for k in ('x', 'w1', 'b1', 'w2', 'b2'):
        within_rule('grad ' + k, t[k].grad.cpu().numpy(), c['32'][k], c['64'][k])


def test_relu_output_into_another_consumer():
    """A ReLU layer whose output does not feed ops.linear masks its gradient itself."""
    c = mlp_case()
    t = dict((k, _dev(v).requires_grad_(k != 'g')) for k, v in c['arrs'].items())
    _lib.TRACE = trace = []
    try:
        h = ops.linear(t['x'], t['w1'], t['b1'], relu=True)
        (h * t['g'][:, :1]).sum().backward()
    finally:
        _lib.TRACE = None
    assert trace.count('cy_act_bwd') == 1
    within_rule('grad x', t['x'].grad.cpu().numpy(), c['32']['x_alone'], c['64']['x_alone'])
    with torch.no_grad():                                     # no graph: nothing is saved, nothing is claimed
        h2 = ops.linear(t['x'], t['w1'], t['b1'], relu=True)
        y2 = ops.linear(h2, t['w2'], t['b2'])
    assert torch.equal(h2, h.detach()) and not y2.requires_grad


def test_unaligned_views_are_copied():
    c = int_case(17, 43, 128)
    base = torch.zeros(17 * 128 + 1, dtype=torch.float32, device='cuda')
    x = base[1:].view(17, 128)
    x.copy_(_dev(c['x']))
    assert x.data_ptr() % 16 != 0
    y = ops.linear(x, _dev(c['w']), _dev(c['b']))
    np.testing.assert_array_equal(y.cpu().numpy(), (c['z'] + c['b']).astype(np.float32))


# ------------------------------------------------------------------------------------------------ softmax cross-entropy
XENT = [(1, 1), (1, 43), (4, 43), (130, 3), (64, 1000)]


@functools.lru_cache(maxsize=None)
def xent_case(M, C, mag):
    rng = np.random.default_rng(50 + M + C)
    s = rng.standard_normal((M, C)).astype(np.float32)
    if mag:
        s = (mag * np.sign(s) + s).astype(np.float32)
    y = rng.integers(0, C, M).astype(np.int64)
    out = dict(s=s, y=y)
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        ts = torch.from_numpy(s).to(dt).requires_grad_(True)
        loss = F.cross_entropy(ts, torch.from_numpy(y))
        loss.backward()
        out['loss' + tag], out['grad' + tag] = loss.item(), ts.grad.numpy()
    return out


def _xent(c, scale=None):
    s = _dev(c['s']).requires_grad_(True)
    loss = ops.softmax_xent_fn(s, torch.from_numpy(c['y']).cuda())
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), s.grad


@pytest.mark.parametrize('M,C', XENT)
def test_softmax_xent_against_fp64(M, C):
    c = xent_case(M, C, 0)
    loss, grad = _xent(c)
    assert loss.shape == () and grad.shape == (M, C)
    within_rule('loss', loss.item(), c['loss32'], c['loss64'])
    within_rule('dscores', grad.cpu().numpy(), c['grad32'], c['grad64'])
    again = _xent(c)
    assert torch.equal(loss.view(torch.int32), again[0].view(torch.int32)) and torch.equal(grad.view(torch.int32), again[1].view(torch.int32))
    half = _xent(c, 0.5)                                                 # an upstream gradient of 0.5: exactly half
    np.testing.assert_array_equal(half[1].cpu().numpy(), grad.cpu().numpy() * np.float32(0.5))


@pytest.mark.parametrize('mag', [80, 100])
@pytest.mark.parametrize('M,C', [(4, 43), (64, 1000)])
def test_softmax_xent_large_logits(M, C, mag):
    """Logits of magnitude 80 and 100: exp(100) is no fp32 number, so the loss is finite only with the row maximum subtracted."""
    c = xent_case(M, C, mag)
    loss, grad = _xent(c)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    within_rule('loss', loss.item(), c['loss32'], c['loss64'])
    within_rule('dscores', grad.cpu().numpy(), c['grad32'], c['grad64'])

"""The general routing kernels (csrc/routing_general.hip) against the fp64 oracle at the tolerances of test_routing_vs_oracle:
shapes outside the specialised kernels' set, the forced-general path on the specialised shapes, the shared s_hist between the two
paths, run-to-run bit identity, and the launch census of the built shapes."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import load_golden, routing_case

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    return torch.device('cuda:0')


def close(a, b, rtol, atol):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


@pytest.fixture
def force_general():
    from capsyolo_amd import ops
    ops.ROUTING_FORCE_GENERAL = True
    yield
    ops.ROUTING_FORCE_GENERAL = False


def oracle_case(shape, seed=11):
    from oracle.models import dynamic_routing
    R, N, Cc, Din, Dout, n_iter = shape
    u, W, G = rnd((R, N, Din), seed, 0.8), rnd((1, N, Cc, Din, Dout), seed + 1, 0.15), rnd((R, Cc, Dout), seed + 2)
    ur, Wr = u.double().requires_grad_(True), W.double().requires_grad_(True)
    vr = dynamic_routing(ur, Wr, n_iter)
    (vr * G.double()).sum().backward()
    return u, W, G, vr, ur.grad, Wr.grad


def hip_case(u, W, G, n_iter):
    from capsyolo_amd import ops
    ut, Wt = u.to(dev()).requires_grad_(True), W.to(dev()).requires_grad_(True)
    v = ops.routing(ut, Wt, n_iter)
    (v * G.to(dev())).sum().backward()
    return v.detach(), ut.grad, Wt.grad


def check(shape):
    u, W, G, vr, dur, dWr = oracle_case(shape)
    v, du, dW = hip_case(u, W, G, shape[-1])
    close(v, vr, 1e-4, 1e-5)
    close(du, dur, 1e-3, 1e-4)
    close(dW, dWr, 1e-3, 1e-4)


# (R, N, C, Din, Dout, n_iter): every Din in {1, 4, 16}, Dout in {1, 3, 15, 17, 32, 64}, C in {2, 65, 100, 256}, N in {1, 37, 1296},
# n_iter in {1, 2, 3, 7}; few rows (several chunks of input capsules, split row sums of dW) and many rows
GENERAL_SHAPES = [
    (5, 37, 2, 1, 1, 1), (7, 37, 65, 4, 3, 2), (3, 37, 100, 16, 15, 3), (2, 37, 256, 4, 17, 7), (4, 1, 100, 16, 32, 3),
    (2, 37, 256, 16, 64, 2), (32, 1296, 2, 4, 3, 3), (3, 1296, 65, 1, 17, 2), (16, 37, 43, 16, 32, 3), (9, 20, 7, 4, 64, 7),
    (1000, 1, 65, 16, 15, 3), (1024, 4, 100, 4, 32, 2), (1100, 3, 256, 1, 1, 7), (1000, 2, 2, 16, 64, 3), (1030, 5, 17, 4, 21, 1),
    (1200, 3, 130, 4, 3, 3),
]


@pytest.mark.parametrize('shape', GENERAL_SHAPES)
def test_general_routing_vs_oracle(shape):
    from capsyolo_amd import _lib
    R, N, Cc, Din, Dout, n_iter = shape
    a = _lib.RoutingFwd(R=R, N=N, C=Cc, Din=Din, Dout=Dout, n_iter=n_iter)
    assert _lib.query('cy_routing_specialised', ctypes.byref(a)) == 0
    check(shape)


@pytest.mark.parametrize('C,Dout,n_iter', [(80, 21, 3), (43, 21, 2), (2, 5, 1)])
def test_general_routing_cell_gather(C, Dout, n_iter, force_general):
    """The cell gather read in place from the NHWC feature map (DarkCapsuleNet3 with 80 classes) == cell_gather + oracle routing."""
    from capsyolo_amd import ops
    from oracle.models import cell_gather, dynamic_routing
    g, B = 2, 2
    feat = rnd((B, 256, 4 * g, 4 * g), 21, 0.7)
    W = rnd((1, 512, C, 8, Dout), 22, 0.1)
    fr, Wr = feat.double().requires_grad_(True), W.double().requires_grad_(True)
    vr = dynamic_routing(cell_gather(fr, g), Wr, n_iter).reshape(g, g, B, C, Dout).permute(2, 0, 1, 3, 4)
    G = rnd(tuple(vr.shape), 23)
    (vr * G.double()).sum().backward()
    fh = feat.permute(0, 2, 3, 1).contiguous().to(dev()).requires_grad_(True)
    Wh = W.to(dev()).requires_grad_(True)
    v = ops.routing(fh, Wh, n_iter, g, B)
    (v * G.to(dev())).sum().backward()
    close(v, vr, 1e-4, 1e-5)
    close(fh.grad.permute(0, 3, 1, 2), fr.grad, 1e-3, 1e-4)
    close(Wh.grad, Wr.grad, 1e-3, 1e-4)


ORACLE_SHAPES = [(37, 70, 43, 8, 16, 3), (9, 33, 7, 8, 21, 2), (130, 512, 1, 8, 5, 3), (5, 64, 64, 8, 16, 3), (3, 20, 3, 8, 5, 4),
                 (1100, 12, 5, 8, 16, 3), (600, 10, 7, 8, 21, 2), (1030, 9, 3, 8, 5, 3), (1100, 20, 43, 8, 21, 4),
                 (1100, 16, 20, 8, 16, 5), (1050, 8, 6, 8, 21, 6), (1040, 10, 49, 8, 48, 2), (32, 1296, 43, 8, 16, 3),
                 (6, 40, 49, 8, 48, 3), (5, 30, 4, 8, 48, 2), (4, 24, 20, 8, 48, 3), (70, 300, 43, 8, 21, 3), (200, 64, 33, 8, 16, 3)]


@pytest.mark.parametrize('shape', ORACLE_SHAPES)
def test_forced_general_on_the_specialised_shapes(shape, force_general):
    check(shape)


@pytest.mark.parametrize('ci', [0, 1, 2, 3])
@pytest.mark.parametrize('n_iter', [1, 3])
def test_forced_general_routing_golden(ci, n_iter, force_general):
    """The reference's own outputs / gradients (tests/golden/routing.npz) on the general kernels."""
    from capsyolo_amd import ops
    from helpers import grad_digest
    g = load_golden('routing')
    R, N, Cc, Din, Dout = (int(v) for v in g['c%d_shape' % ci])
    u, W, G = routing_case(ci, R, N, Cc, Din, Dout)
    ut = T(u).to(dev()).requires_grad_(True)
    Wt = T(W).to(dev()).requires_grad_(True)
    v = ops.routing(ut, Wt, n_iter)
    (v * T(G).to(dev())).sum().backward()
    key = 'c%d_r%d_' % (ci, n_iter)
    close(v, g[key + 'v'], 1e-4, 1e-5)
    close(ut.grad, g[key + 'du'], 1e-3, 1e-4)
    close(grad_digest(Wt.grad.cpu()), g[key + 'dW_digest'], 1e-3, 1e-4)


@pytest.mark.parametrize('shape', [(32, 1296, 43, 8, 16, 3), (1100, 20, 43, 8, 21, 4), (6, 40, 49, 8, 48, 3), (130, 512, 1, 8, 5, 3)])
@pytest.mark.parametrize('fwd_general', [False, True])
def test_forward_on_one_path_feeds_backward_on_the_other(shape, fwd_general):
    """s_hist has one layout and meaning on both paths: a specialised forward + general backward, and the reverse."""
    from capsyolo_amd import ops
    u, W, G, vr, dur, dWr = oracle_case(shape)
    ut, Wt = u.to(dev()).requires_grad_(True), W.to(dev()).requires_grad_(True)
    try:
        ops.ROUTING_FORCE_GENERAL = fwd_general
        v = ops.routing(ut, Wt, shape[-1])
        ops.ROUTING_FORCE_GENERAL = not fwd_general
        (v * G.to(dev())).sum().backward()
    finally:
        ops.ROUTING_FORCE_GENERAL = False
    close(v, vr, 1e-4, 1e-5)
    close(ut.grad, dur, 1e-3, 1e-4)
    close(Wt.grad, dWr, 1e-3, 1e-4)


@pytest.mark.parametrize('shape', [(32, 1296, 100, 8, 16, 3), (1200, 16, 80, 8, 21, 3), (7, 37, 256, 16, 64, 4)])
def test_general_routing_is_bit_identical_run_to_run(shape):
    R, N, Cc, Din, Dout, n_iter = shape
    u, W, G = rnd((R, N, Din), 41, 0.8), rnd((1, N, Cc, Din, Dout), 42, 0.15), rnd((R, Cc, Dout), 43)
    a, b = hip_case(u, W, G, n_iter), hip_case(u, W, G, n_iter)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_built_shapes_call_only_the_specialised_entry_points():
    """Launch census (_lib.TRACE): every built shape still goes through cy_routing_fwd / cy_routing_bwd, other shapes through the
    general entry points."""
    from capsyolo_amd import _lib, ops
    built = [(40, 512, 1, 8, 5, 2), (32, 1296, 43, 8, 16, 3), (300, 512, 43, 8, 21, 3), (32, 784, 49, 8, 48, 3)] + ORACLE_SHAPES
    for shape, want in [(s, {'cy_routing_fwd', 'cy_routing_bwd'}) for s in built] + \
                       [((32, 50, 100, 8, 16, 3), {'cy_routing_general_fwd', 'cy_routing_general_bwd'})]:
        R, N, Cc, Din, Dout, n_iter = shape
        u = rnd((R, N, Din), 1).to(dev()).requires_grad_(True)
        W = rnd((1, N, Cc, Din, Dout), 2, 0.1).to(dev()).requires_grad_(True)
        _lib.TRACE = []
        try:
            v = ops.routing(u, W, n_iter)
            v.sum().backward()
        finally:
            trace, _lib.TRACE = _lib.TRACE, None
        assert set(n for n in trace if 'routing' in n) == want, (shape, trace)


@pytest.mark.parametrize('shape', [(4, 10, 300, 8, 16, 3), (4, 10, 43, 17, 16, 3), (4, 10, 43, 8, 65, 3)])
def test_outside_the_envelope_is_an_error(shape):
    from capsyolo_amd import _lib, ops
    R, N, Cc, Din, Dout, n_iter = shape
    u, W = rnd((R, N, Din), 1).to(dev()), rnd((1, N, Cc, Din, Dout), 2).to(dev())
    with pytest.raises(_lib.HipExtensionError, match='envelope'):
        ops.routing(u, W, n_iter)


# ------------------------------------------------------------------------------------------------ the workspace stays inside the plan's total
GUARD, PATTERN = 1024, 0x5A5A5A5A        # floats before and after the workspace (a multiple of 4: the slice keeps its 16-byte alignment)


def guarded_ws(total):
    buf = torch.full((GUARD + total + GUARD,), PATTERN, dtype=torch.int32, device=dev())
    return buf, buf.view(torch.float32)[GUARD:GUARD + total]


def guards_untouched(buf, total):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + total:] == PATTERN).all())


def guard_case(shape, g=0, B=0, want_path=None):
    """cy_routing_fwd / _bwd (or the general entry points, as the plan says) called directly on a workspace of exactly the plan's
    total floats cut out of a larger tensor: the 1024 floats on either side keep their bit pattern, and the results are those of
    ops.routing on the same inputs."""
    from capsyolo_amd import _lib, ops
    R, N, Cc, Din, Dout, n_iter = shape
    if g:
        u, out_shape = rnd((B, 4 * g, 4 * g, 256), 51, 0.7).to(dev()), (B, g, g, Cc, Dout)
    else:
        u, out_shape = rnd((R, N, Din), 51, 0.8).to(dev()), (R, Cc, Dout)
    W, G = rnd((1, N, Cc, Din, Dout), 52, 0.15).to(dev()), rnd(out_shape, 53).to(dev())
    ur, Wr = u.clone().requires_grad_(True), W.clone().requires_grad_(True)
    vr = ops.routing(ur, Wr, n_iter, g, B)
    (vr * G).sum().backward()

    pf, pb = ops.routing_plan(*shape, g, B), ops.routing_plan(*shape, g, B, backward=True)
    if want_path:
        assert pf['path'] == want_path, pf
    entry = 'cy_routing_general_' if pf['path'] == 'general' else 'cy_routing_'
    v, s_hist = torch.empty(out_shape, device=dev()), torch.empty((n_iter, R, Cc, Dout), device=dev())
    buf, ws = guarded_ws(pf['total'])
    a = _lib.RoutingFwd(u=u.data_ptr(), W=W.data_ptr(), v_out=v.data_ptr(), s_hist=s_hist.data_ptr(), R=R, N=N, C=Cc, Din=Din, Dout=Dout,
                        n_iter=n_iter, gather_g=g, gather_B=B, ws=ws.data_ptr() if pf['total'] else None)
    _lib.call(entry + 'fwd', ctypes.byref(a), ops._stream())
    torch.cuda.synchronize()
    assert guards_untouched(buf, pf['total']), ('forward', shape, pf)
    assert torch.equal(v, vr.detach())

    du, dW = torch.empty_like(u), torch.empty_like(W)
    buf, ws = guarded_ws(pb['total'])
    a = _lib.RoutingBwd(u=u.data_ptr(), W=W.data_ptr(), s_hist=s_hist.data_ptr(), dv=G.data_ptr(), du=du.data_ptr(), dW=dW.data_ptr(),
                        ws=ws.data_ptr(), R=R, N=N, C=Cc, Din=Din, Dout=Dout, n_iter=n_iter, gather_g=g, gather_B=B)
    _lib.call(entry + 'bwd', ctypes.byref(a), ops._stream())
    torch.cuda.synchronize()
    assert guards_untouched(buf, pb['total']), ('backward', shape, pb)
    assert torch.equal(du, ur.grad)
    if pb['path'] in ('c1', 'general'):
        assert torch.equal(dW, Wr.grad)
    else:
        # routing_caps.hip adds its row chunks into dW with float atomics: the same partial sums in another order.  Reordering a
        # sum of K <= 256 fp32 terms moves it by at most K * 2^-24 * sum |terms|; 1e-5 of the largest |dW| is 168 * 2^-24 of it.
        close(dW, Wr.grad, 0, 1e-5 * float(Wr.grad.abs().max()))
    return pf, pb


@pytest.mark.parametrize('shape,g,B,path', [
    ((130, 512, 1, 8, 5, 3), 0, 0, 'c1'), ((1100, 12, 5, 8, 16, 3), 0, 0, 'rows_fused'), ((37, 70, 43, 8, 16, 3), 0, 0, 'rows_phased'),
    ((6, 40, 49, 8, 48, 2), 0, 0, 'rows_phased'), ((45, 512, 1, 8, 5, 3), 3, 5, 'c1'), ((9, 20, 7, 4, 64, 7), 0, 0, 'general'),
    ((1200, 3, 130, 4, 3, 3), 0, 0, 'general')])
def test_workspace_stays_inside_the_plan_total(shape, g, B, path):
    guard_case(shape, g, B, path)


def test_workspace_stays_inside_the_plan_total_on_the_mfma_forward():
    """The same check in a fresh process that has CY_ROUTING_MFMA=1 from its start."""
    import os
    import subprocess
    import sys
    from helpers import REPO
    code = ('import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_routing_general as t\n'
            't.guard_case((37, 70, 43, 8, 16, 3), want_path="mfma_phased")\nprint("guards ok")\n' % (REPO, os.path.join(REPO, 'tests')))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, CY_ROUTING_MFMA='1'), capture_output=True, text=True)
    assert r.returncode == 0 and 'guards ok' in r.stdout, r.stdout + r.stderr

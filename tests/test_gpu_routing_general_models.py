"""Models whose routing head the specialised kernels do not take (n_classes > 64, n_grid = 9, other widths) run end to end on the
general routing kernels: every parameter gradient against the oracle models in fp64, as test_models_vs_fp64_oracle measures."""
import copy

import numpy as np
import pytest
import torch

from helpers import make_params, synth_gtsdb_labels, synth_images

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _vs_fp64(o32, hip, f_o, f_h):
    """HIP vs the oracle in fp64 from the same initialisation, with the oracle's own fp32 error as the yardstick."""
    hip.load_state_dict(o32.state_dict())
    o64 = copy.deepcopy(o32).double()
    o32.train(), o64.train(), hip.cuda().train()
    out64, l64 = f_o(o64, torch.float64)
    l64.backward()
    out32, l32 = f_o(o32, torch.float32)
    l32.backward()
    outh, lh = f_h(hip)
    lh.backward()
    assert _rel_l2(outh, out64) <= max(1e-4, 20 * _rel_l2(out32, out64))
    assert abs(lh.item() - l64.item()) <= 1e-4 * abs(l64.item())
    g64 = dict((n, q.grad) for n, q in o64.named_parameters())
    g32 = dict((n, q.grad) for n, q in o32.named_parameters())
    n_checked = 0
    for n, q in hip.named_parameters():
        if g64[n] is None:
            assert q.grad is None, n
            continue
        if '.conv_' in n and n.endswith('bias'):
            continue
        e_h, e_32 = _rel_l2(q.grad, g64[n]), _rel_l2(g32[n], g64[n])
        assert e_h <= max(2e-2, 20 * e_32), '%s: HIP %.2e vs reference-fp32 %.2e (relative L2 against fp64)' % (n, e_h, e_32)
        n_checked += 1
    assert n_checked > 0


def _routing_calls(fn):
    from capsyolo_amd import _lib
    _lib.TRACE = []
    try:
        fn()
    finally:
        trace, _lib.TRACE = _lib.TRACE, None
    return set(n for n in trace if 'routing' in n)


@pytest.mark.parametrize('recon', [False, True])
def test_capsule_net_100_classes(recon):
    from capsyolo_amd import loss_fns, models
    from oracle import loss_fns as OL
    from oracle import models as OM
    torch.manual_seed(0)
    p = make_params(model='capsule', n_classes=100, recon=recon, device='cuda')
    x, y = T(synth_images(8, 32, seed=42)), T(np.arange(8, dtype=np.int64) * 12)

    def f_o(net, dt):
        if not recon:
            s = net(x.to(dt))
            return s, OL.capsule_loss(s, y, p)
        s, r = net(x.to(dt), y, True)
        return s, OL.capsule_loss(s, y, p, x.to(dt), r)

    def f_h(net):
        if not recon:
            s = net(x.cuda())
            return s, loss_fns.capsule_loss(s, y.cuda(), p)
        s, r = net(x.cuda(), y.cuda(), True)
        return s, loss_fns.capsule_loss(s, y.cuda(), p, x.cuda(), r)
    calls = _routing_calls(lambda: _vs_fp64(OM.CapsuleNet(p), models.CapsuleNet(p), f_o, f_h))
    assert calls == {'cy_routing_general_fwd', 'cy_routing_general_bwd'}, calls


def test_darkcapsule3_net_80_classes():
    from capsyolo_amd import loss_fns, models
    from oracle import loss_fns as OL
    from oracle import models as OM
    torch.manual_seed(0)
    p = make_params(model='darkcapsule3', n_grid=2, n_classes=80, darknet_input=64, recon=False, device='cuda')
    x, y = T(synth_images(2, 64, seed=22)), T(synth_gtsdb_labels(2, 2, 80, seed=24))
    f_o = lambda net, dt: (lambda o: (o, OL.darkcapsule3_loss(o, y.to(dt), p)))(net(x.to(dt)))
    f_h = lambda net: (lambda o: (o, loss_fns.darkcapsule3_loss(o, y.cuda(), p)))(net(x.cuda()))
    calls = _routing_calls(lambda: _vs_fp64(OM.DarkCapsuleNet3(p), models.DarkCapsuleNet3(p), f_o, f_h))
    assert calls == {'cy_routing_general_fwd', 'cy_routing_general_bwd'}, calls


def test_darkcapsule2_net_9x9_grid():
    from capsyolo_amd import loss_fns, models
    from oracle import loss_fns as OL
    from oracle import models as OM
    torch.manual_seed(0)
    p = make_params(model='darkcapsule2', n_grid=9, n_classes=10, darknet_input=224, recon=False, dropout=0.0, device='cuda')
    x, y = T(synth_images(2, 224, seed=32)), T(synth_gtsdb_labels(2, 9, 10, seed=33))
    f_o = lambda net, dt: (lambda o: (o, OL.darkcapsule2_loss(o, y.to(dt), p)))(net(x.to(dt)))
    f_h = lambda net: (lambda o: (o, loss_fns.darkcapsule2_loss(o, y.cuda(), p)))(net(x.cuda()))
    calls = _routing_calls(lambda: _vs_fp64(OM.DarkCapsuleNet2(p), models.DarkCapsuleNet2(p), f_o, f_h))
    assert calls == {'cy_routing_general_fwd', 'cy_routing_general_bwd'}, calls


def test_main_capsule_100_classes_graph_equals_eager(tmp_path):
    """main.py --model capsule --synthetic with 100 classes trains, and the HIP-graph-captured step (the general routing kernels
    inside the capture) gives the eager loop's epoch losses."""
    import importlib.util
    import json
    import os
    from helpers import REPO
    spec = importlib.util.spec_from_file_location('cy_main', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    cfg = dict(batch_size=8, n_epochs=2, n_classes=100, lr_decay=0.1, capsule_input=32)
    out = {}
    for mode in ('eager', 'graph'):
        mdir = str(tmp_path / mode)
        os.makedirs(mdir)
        json.dump(cfg, open(os.path.join(mdir, 'params.json'), 'w'))
        argv = ['--model', 'capsule', '--synthetic', '20', '--model_dir', mdir, '--fix_ckpt_dir'] + (['--graph'] if mode == 'graph' else [])
        out[mode] = m.main(argv)
    assert np.all(np.isfinite(np.asarray(out['eager'][0], dtype=np.float64)))
    np.testing.assert_allclose(out['graph'][0], out['eager'][0], rtol=2e-4)
    np.testing.assert_allclose(out['graph'][1], out['eager'][1], rtol=2e-4)

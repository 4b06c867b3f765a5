"""ConvNet on the project's kernels (params.json "cnn_kernels": "hip"): the conv blocks, the flatten transpose, the linear kernels
of csrc/linear.hip, the cross-entropy kernel and optim.Adam against the reference's goldens (tests/golden/models.npz) and against
the oracle run in float64 on the CPU inside the tests."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, closed_form_state, grad_digest, load_golden, make_params, synth_images

from capsyolo_amd import loss_fns, models, optim, predict_fns, serve, synth
from oracle import loss_fns as OL
from oracle import models as OM

pytestmark = pytest.mark.gpu
T = torch.from_numpy
BN_FED_BIASES = ('cnn.0.bias', 'cnn.4.bias')
STEPS = 12


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol)


def _digest_err(a, b):
    a, b = np.asarray(a, dtype=np.float64)[2:], np.asarray(b, dtype=np.float64)[2:]
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _params(**kw):
    return make_params(model='cnn', cnn_kernels='hip', device='cuda', **kw)


def _hip_net(p):
    net = models.ConvNet(p)
    net.load_state_dict(closed_form_state(net))
    return net.cuda()


def _golden_batch():
    return T(synth_images(4, 32, seed=21)), T(np.array([3, 42, 0, 17], dtype=np.int64))


class _Oracle64(object):
    """The oracle's ConvNet in float64 on the CPU, on the golden batch: the gradient digests of one step, the loss curve of STEPS
    Adam steps, and the net after those steps.  Computed once for the module."""

    def __init__(self):
        x, y = _golden_batch()
        x = x.double()
        p = make_params(model='cnn', dropout=0.0)
        net = OM.ConvNet(p)
        net.load_state_dict(closed_form_state(net))
        net.double().train()
        loss = OL.cnn_loss(net(x), y)
        loss.backward()
        self.digest = dict((n, grad_digest(q.grad)) for n, q in net.named_parameters())
        net = OM.ConvNet(p)
        net.load_state_dict(closed_form_state(net))
        net.double().train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        self.curve = []
        for _ in range(STEPS):
            loss = OL.cnn_loss(net(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            self.curve.append(loss.item())
        self.curve = np.array(self.curve)
        self.net = net


@pytest.fixture(scope='module')
def oracle64():
    return _Oracle64()


def test_golden_step(oracle64):
    g = load_golden('models')
    p = _params(dropout=0.0)
    x, y = (t.cuda() for t in _golden_batch())
    net = _hip_net(p).train()
    out = net(x)
    loss = loss_fns.cnn_loss(out, y, p)
    loss.backward()
    close(out.detach().cpu().numpy(), g['cnn_out'], 2e-4, 2e-5)
    close(loss.item(), g['cnn_loss'], 2e-4, 1e-6)
    grads = dict((n, q.grad) for n, q in net.named_parameters())
    assert all(v is not None for v in grads.values()) and len(grads) == 12
    for name, grad in grads.items():
        if name in BN_FED_BIASES:              # noise-only in the reference (a bias in front of a BatchNorm)
            w = grads[name[:-len('bias')] + 'weight']
            assert float(grad.abs().max()) <= 1e-4 * float(w.abs().max()), name
            continue
        ref64 = oracle64.digest[name]
        e_hip, e_32 = _digest_err(grad_digest(grad.cpu()), ref64), _digest_err(g['cnn_grad/' + name], ref64)
        print('%s: HIP %.3e, reference fp32 %.3e (relative L2 of the digest against the fp64 oracle)' % (name, e_hip, e_32))
        assert e_hip <= max(2e-3, 20 * e_32), '%s: HIP %.3e vs reference fp32 %.3e' % (name, e_hip, e_32)
    for name, b in net.named_buffers():
        if name.endswith('running_mean') or name.endswith('running_var'):
            ref = g['cnn_buf/' + name]
            close(b.cpu().numpy(), ref, 2e-4, 2e-4 * float(np.abs(ref).max()))
    assert int(net.cnn[1].num_batches_tracked) == 1 and int(net.cnn[5].num_batches_tracked) == 1


@pytest.fixture(scope='module')
def trained(oracle64):
    """STEPS Adam steps of the HIP model on the golden batch: (net, params, loss curve)."""
    p = _params(dropout=0.0)
    x, y = (t.cuda() for t in _golden_batch())
    net = _hip_net(p).train()
    opt = optim.Adam([q for q in net.parameters() if q.requires_grad], lr=1e-3)
    curve = []
    for _ in range(STEPS):
        loss = loss_fns.cnn_loss(net(x), y, p)
        opt.zero_grad()
        loss.backward()
        opt.step()
        curve.append(loss.item())
    return net, p, np.array(curve)


def test_curve(trained, oracle64):
    curve, ref = trained[2], oracle64.curve
    span = float(ref.max() - ref.min())
    print('HIP   : %s\noracle: %s\nlargest deviation %.3e of the range' % (curve, ref, np.abs(curve - ref).max() / span))
    assert ref[-1] < ref[0]
    close(curve[0], ref[0], 2e-4, 1e-6)
    close(curve, ref, 0.0, 1e-2 * span)
    close(curve[-1], ref[-1], 0.0, 5e-3 * span)


def test_eval_after_training(trained, oracle64):
    net, p, _ = trained
    x = T(synth_images(16, 32, seed=33))
    state = dict((k, v.detach().cpu()) for k, v in net.state_dict().items())
    ref = OM.ConvNet(make_params(model='cnn', dropout=0.0))
    ref.load_state_dict(state)
    ref.double().eval()
    plain = models.ConvNet(make_params(model='cnn', dropout=0.0, device='cuda'))
    plain.load_state_dict(state)
    plain.cuda().eval()
    net.eval()
    try:
        with torch.no_grad():
            want = ref(x.double()).numpy()
            got = net(x.cuda()).cpu().numpy()
            torch_gpu = plain(x.cuda()).cpu().numpy()
    finally:
        net.train()
    top = np.sort(want, axis=1)
    print('smallest gap between the two best classes (fp64): %.3e' % (top[:, -1] - top[:, -2]).min())
    close(got, want, 2e-4, 2e-5)
    np.testing.assert_array_equal(np.argmax(got, axis=1), np.argmax(torch_gpu, axis=1))


def test_dropout_on_torchs_rng():
    x, y = (t.cuda() for t in _golden_batch())

    def step(dropout):
        p = _params(dropout=dropout)
        net = _hip_net(p).train()
        torch.manual_seed(1234)
        loss = loss_fns.cnn_loss(net(x), y, p)
        loss.backward()
        return loss.item(), [q.grad.clone() for q in net.parameters()]
    a, b, plain = step(0.5), step(0.5), step(0.0)
    assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1], b[1]))
    assert np.isfinite(a[0]) and a[0] != plain[0]


# ------------------------------------------------------------------------------------------------ the streaming detector
K_PIPE = 8


def _frames(seed, h=80, w=100, n=2):
    return [im[:h, :w] for im in synth.raw_images(n, seed=seed, min_side=max(h, w), max_side=160)]


def test_serve_with_the_hip_classifier():
    """serve.SignDetector on the shapes of tests/test_gpu_serve.py (two 80 x 100 frames, DarkNet at 64, 8 box slots)."""
    dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    torch.manual_seed(3)
    dark = models.DarkNet(dp).cuda().eval()
    frames = _frames(41)
    with torch.no_grad():
        yd = dark(predict_fns.PackedImages(frames).resize(64, to_nchw=True)).data
    conf = np.unique(yd[..., 0::5].cpu().numpy())[::-1].astype(np.float64)
    assert len(conf) >= 7
    conf_th = float(conf[4] + conf[5]) / 2
    cp = _params(n_classes=3, dropout=0.0)
    torch.manual_seed(5)
    cnn = models.ConvNet(cp).cuda()
    eager = serve.SignDetector(dark, dp, cnn, cp, max_boxes=K_PIPE, conf_th=conf_th)
    graphed = serve.SignDetector(dark, dp, cnn, cp, max_boxes=K_PIPE, conf_th=conf_th, graph=True)
    a, b = eager.detect(frames), graphed.detect(frames)
    np.testing.assert_array_equal(b.record, a.record)
    np.testing.assert_array_equal(graphed.detect(frames).record, a.record)             # a replay after the capturing call
    assert 1 <= a.n <= K_PIPE - 1 and (a.classes >= 0).all() and (a.classes < 3).all()
    # the same weights in the plain-torch model: the same boxes, and the same classes where the arg-max is clear
    plain = models.ConvNet(make_params(model='cnn', n_classes=3, dropout=0.0, device='cuda'))
    plain.load_state_dict(cnn.state_dict())
    c = serve.SignDetector(dark, dp, plain.cuda(), make_params(model='cnn', n_classes=3, dropout=0.0, device='cuda'),
                           max_boxes=K_PIPE, conf_th=conf_th).detect(frames)
    np.testing.assert_array_equal(c.boxes_xy, a.boxes_xy)
    np.testing.assert_allclose(c.class_scores, a.class_scores, rtol=2e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------------ the command line
def test_main_trains_with_the_step_as_a_graph(tmp_path):
    spec = importlib.util.spec_from_file_location('cy_main_convnet', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    mdir = str(tmp_path / 'cnn')
    os.makedirs(mdir)
    json.dump(dict(batch_size=16, n_epochs=2, n_classes=43, lr_decay=0.1, dropout=0.0), open(os.path.join(mdir, 'params.json'), 'w'))
    losses_tr, losses_ev = m.main(['--model', 'cnn', '--cnn_kernels', 'hip', '--synthetic', '64', '--n_epochs', '2', '--graph', '--no_metric',
                                   '--fix_ckpt_dir', '--model_dir', mdir])
    print('train %s eval %s' % (losses_tr, losses_ev))
    assert len(losses_tr) == 2 and np.all(np.isfinite(losses_tr)) and np.all(np.isfinite(losses_ev))
    assert losses_tr[1] < losses_tr[0]
    ck = torch.load(os.path.join(mdir, 'last.pth.tar'), map_location='cpu', weights_only=False)
    plain = models.ConvNet(make_params(model='cnn'))
    plain.load_state_dict(ck['state_dict'])                                # strict: the plain-torch model takes the checkpoint
    assert type(plain.cnn[0]) is torch.nn.Conv2d and int(plain.cnn[1].num_batches_tracked) > 0

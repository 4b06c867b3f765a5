"""Host side of the linear kernels and of ConvNet on them (csrc/linear.hip, params.json "cnn_kernels"): the share rule of the
forward's split reduction, the refusals in front of any launch, the model's state_dict against the oracle's, the switch and the
command line without a GPU.  No GPU is needed."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import REPO, closed_form_state, make_params

from capsyolo_amd import _lib, loss_fns, models, ops
from oracle import models as OM


def _main_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_share_rule_without_a_device():
    assert ops.linear_shares(17, 43, 128) == (1, 128, 0)                 # K fits one slice: one share, no workspace
    assert ops.linear_shares(1, 1, 4)[0] == 1
    for M in (16, 64, 4, 1024):
        shares, slice_, ws = ops.linear_shares(M, 128, 32768)
        print('M=%d: %d shares of %d' % (M, shares, slice_))
        assert 1 < shares <= 256 and slice_ % 64 == 0
        assert shares * slice_ >= 32768 > (shares - 1) * slice_          # every share holds a part of K
        assert ws == shares * M * 128
        assert 4 * ws <= 128 * 32768                                     # the partial sums: at most a quarter of W
    # the exported names exist and answer -1 outside the range
    assert _lib.query('cy_linear_fwd_shares', 16, 128, 130) == -1 and _lib.query('cy_linear_fwd_ws_floats', 5000, 128, 128) == -1
    assert _lib.query('cy_linear_fwd_slice', 16, 2000, 128) == -1
    for name in ('cy_linear_fwd', 'cy_linear_dgrad', 'cy_linear_wgrad', 'cy_softmax_xent', 'cy_linear_fwd_shares',
                 'cy_linear_fwd_slice', 'cy_linear_fwd_ws_floats'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    assert 'cy_linear_fwd_ws_floats' in header and 'cy_softmax_xent' in header
    assert _lib.load().capsyolo_abi_version() == 6


def test_refusals_before_any_launch():
    E = _lib.HipExtensionError
    with pytest.raises(E, match='GPU'):                                  # CPU tensors, as everywhere else
        ops.linear(torch.zeros(4, 128), torch.zeros(8, 128), torch.zeros(8))
    with pytest.raises(E, match='GPU'):
        ops.softmax_xent_fn(torch.zeros(4, 43), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(E, match='K=130'):
        ops.linear(torch.zeros(4, 130), torch.zeros(8, 130), None)
    with pytest.raises(E, match='N=2000'):
        ops.linear(torch.zeros(4, 128), torch.zeros(2000, 128), None, relu=True)
    with pytest.raises(E, match='M=5000'):
        ops.linear(torch.zeros(5000, 128), torch.zeros(8, 128), None)
    with pytest.raises(E, match='C=0'):
        ops.softmax_xent_fn(torch.zeros(4, 0), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(E, match='C=1025'):
        ops.softmax_xent_fn(torch.zeros(4, 1025), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(E):                                               # shapes that do not fit each other
        ops.linear(torch.zeros(4, 128), torch.zeros(8, 64), None)
    # the library refuses the same shapes itself (null pointers: nothing could be launched)
    for name, args in (('cy_linear_fwd', (None, None, None, None, 4, 8, 130, 0, None, None)),
                       ('cy_linear_dgrad', (None, None, None, None, 4, 2000, 128, None)),
                       ('cy_linear_wgrad', (None, None, None, None, 0, 8, 128, None)),
                       ('cy_softmax_xent', (None, None, None, None, 4, 0, None))):
        with pytest.raises(E, match='outside'):
            _lib.call(name, *args)


def test_hip_convnet_has_the_oracles_state():
    p = make_params(model='cnn', cnn_kernels='hip')
    ref = OM.ConvNet(make_params(model='cnn'))
    net = models.ConvNet(p)
    want, got = ref.state_dict(), net.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    state = closed_form_state(ref)
    net.load_state_dict(state)                                           # strict
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in ref.named_parameters()]
    plain = models.ConvNet(make_params(model='cnn'))
    plain.load_state_dict(net.state_dict())                              # ... and the other way round
    net.load_state_dict(plain.state_dict())
    assert isinstance(net.cnn, models.FusedBackbone) and isinstance(net.cnn[0], models.HipConv2d)
    assert isinstance(net.cnn[10], models.HipLinear) and net.cnn[10].relu and not net.cnn[12].relu
    assert net.cnn[2].slope == 0.01 and net.cnn[6].slope == 0.01         # nn.LeakyReLU's default
    assert isinstance(net.cnn[3], nn.Dropout) and isinstance(net.cnn[8], models.HipMaxPool2)


def test_same_seed_same_initial_weights():
    torch.manual_seed(7)
    a = models.ConvNet(make_params(model='cnn')).state_dict()
    torch.manual_seed(7)
    b = models.ConvNet(make_params(model='cnn', cnn_kernels='hip')).state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_the_switch():
    net = models.ConvNet(make_params(model='cnn'))
    assert type(net.cnn) is nn.Sequential and type(net.cnn[0]) is nn.Conv2d and type(net.cnn[10]) is nn.Linear
    assert type(models.ConvNet(make_params(model='cnn', cnn_kernels='torch')).cnn[0]) is nn.Conv2d
    with pytest.raises(ValueError, match='cnn_kernels'):
        models.ConvNet(make_params(model='cnn', cnn_kernels='fast'))
    # the default loss is the torch expression, on the CPU too
    s = torch.from_numpy(np.random.default_rng(0).standard_normal((4, 43)).astype(np.float32))
    y = torch.tensor([3, 42, 0, 17])
    want = torch.nn.functional.cross_entropy(s, y)
    assert abs(float(loss_fns.cnn_loss(s, y, make_params(model='cnn'))) - float(want)) < 1e-6
    with pytest.raises(_lib.HipExtensionError):                          # 'hip' has no CPU path
        loss_fns.cnn_loss(s, y, make_params(model='cnn', cnn_kernels='hip'))


def test_main_without_a_gpu(tmp_path, monkeypatch):
    m = _main_module('cy_main_linear_host')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)       # load_params decides the device by this
    json.dump(dict(batch_size=8, n_classes=43, n_epochs=1, lr_decay=0.1, dropout=0.0), open(str(tmp_path / 'params.json'), 'w'))
    with pytest.raises(SystemExit, match='no GPU'):
        m.main(['--model', 'cnn', '--cnn_kernels', 'hip', '--synthetic', '8', '--n_epochs', '1', '--no_metric', '--model_dir', str(tmp_path)])
    json.dump(dict(batch_size=8, n_classes=43, n_epochs=1, lr_decay=0.1, dropout=0.0, cnn_kernels='hip'),
              open(str(tmp_path / 'params.json'), 'w'))
    with pytest.raises(SystemExit, match='no GPU'):                      # the key of params.json alone
        m.main(['--model', 'cnn', '--synthetic', '8', '--n_epochs', '1', '--no_metric', '--model_dir', str(tmp_path)])


def test_main_parses_the_switch(tmp_path):
    m = _main_module('cy_main_linear_host2')
    assert m.parser.parse_args([]).cnn_kernels is None
    json.dump(dict(batch_size=8, n_classes=43, cnn_kernels='torch'), open(str(tmp_path / 'params.json'), 'w'))
    args = m.parser.parse_args(['--model', 'cnn', '--cnn_kernels', 'hip'])
    assert m.load_params(str(tmp_path), args).cnn_kernels == 'hip'       # the command line overrides the file
    args = m.parser.parse_args(['--model', 'cnn'])
    assert m.load_params(str(tmp_path), args).cnn_kernels == 'torch'
    args = m.parser.parse_args(['--model', 'capsule', '--cnn_kernels', 'hip'])
    assert m.load_params(str(tmp_path), args).cnn_kernels == 'torch'     # ... for the cnn model only
    with pytest.raises(SystemExit):
        m.parser.parse_args(['--cnn_kernels', 'fast'])

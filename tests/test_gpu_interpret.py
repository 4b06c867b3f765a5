"""GPU tests of capsule interpretation: the fused decoder kernel (csrc/decoder.hip, `cy_decoder_fwd`) behind
capsyolo_amd.interpret, CapsuleNet.capsules and `main.py --mode interpret`.

Tolerance rule of every float comparison: the kernel is compared with oracle.models.CapsuleNet(...).decoder in float64 on the CPU
with the same state dict, and may be max(1e-6, 4 * d32) away from it, d32 being the largest difference between that oracle in
float32 and in float64 on the same inputs (computed here, printed with the measured difference).  The reference's own float32 is
the yardstick; the factor 4 allows for another summation order and for tanhf.

The kernel decodes one vector per workgroup, one workgroup per CU, and loops when there are more vectors than CUs: n = 1000 makes
a workgroup decode several vectors in a row (stale LDS of the previous vector would show), n = 1 and 3 are grids smaller than a
wave's worth of blocks."""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, closed_form_state, grad_digest, load_golden, make_params, synth_images, wave

from capsyolo_amd import _lib, interpret, models, synth, utils
from oracle import models as OM

pytestmark = pytest.mark.gpu

NS = [1, 3, 37, 176, 1000]


def _tol(d32):
    return max(1e-6, 4.0 * d32)


@pytest.fixture(scope='module')
def params():
    return make_params(model='capsule', n_classes=43, device='cuda', batch_size=16)


@pytest.fixture(scope='module')
def net(params):
    m = models.CapsuleNet(params)
    m.load_state_dict(closed_form_state(m))
    return m.cuda().eval()


@pytest.fixture(scope='module')
def oracle(params):
    """the oracle's decoder in float32 and in float64, same state dict"""
    o = OM.CapsuleNet(params)
    o.load_state_dict(closed_form_state(o))
    o.eval()
    return o, copy.deepcopy(o).double()


def _oracle_decode(oracle, t):
    """(float32 run as float64 numpy, float64 run) of the oracle's decoder on float32 vectors t [n,16] (numpy)"""
    o32, o64 = oracle
    with torch.no_grad():
        a = o32.decoder(torch.from_numpy(t)).double().numpy()
        b = o64.decoder(torch.from_numpy(t).double()).numpy()
    return a, b


@pytest.fixture(scope='module')
def dense(oracle):
    """The dense case, computed once at n = 1000: wave() is a function of the flat index, so the first n rows are the case of size n."""
    t = wave((1000, 16), 0.3, amp=1.0, freq=0.913)
    o32, o64 = _oracle_decode(oracle, t)
    return t, o32, o64


@pytest.mark.parametrize('n', NS)
def test_dense_decode_against_fp64(net, dense, n):
    t, o32, o64 = (a[:n] for a in dense)
    assert np.array_equal(t, wave((n, 16), 0.3, amp=1.0, freq=0.913))
    out = interpret.decode_capsules(net, torch.from_numpy(t).cuda())
    assert out.shape == (n, 3, 32, 32) and out.dtype == torch.float32 and out.is_cuda
    d32 = float(np.abs(o32 - o64).max())
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - o64).max())
    print('n = %d: d32 %.3g, kernel vs fp64 %.3g (bound %.3g)' % (n, d32, err, _tol(d32)))
    assert err <= _tol(d32)
    if n == 37:                # tanh saturates: pixels that round to 256 (and to 0) exercise the clamp of the byte output
        q = np.rint(o64 * 128.0 + 128.0)
        assert (q == 256).any() and (q == 0).any() and o64.max() > 0.99 and o64.min() < -0.99


@pytest.mark.parametrize('n', [37, 1000])
def test_u8_mode(net, dense, n):
    t, o32, o64 = (a[:n] for a in dense)
    both = interpret._decode('test', net, torch.from_numpy(t).cuda(), n, 1, f32=True, u8=True)       # ONE launch, both outputs
    f32, u8 = both['f32'].cpu().numpy(), both['u8'].cpu().numpy()
    assert u8.shape == (n, 32, 32, 3) and u8.dtype == np.uint8
    want = np.clip(np.rint(f32 * np.float32(128.0) + np.float32(128.0)), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(u8, want)
    tol = _tol(float(np.abs(o32 - o64).max()))
    off = np.abs(u8.astype(np.float64) - np.clip(o64.transpose(0, 2, 3, 1) * 128.0 + 128.0, 0.0, 255.0))
    print('n = %d: bytes at most %.4f from the unrounded fp64 value (bound %.4f)' % (n, off.max(), 0.5 + 128.0 * tol))
    assert off.max() <= 0.5 + 128.0 * tol
    if n == 37:
        assert (u8 == 255).any() and (u8 == 0).any()
    # the byte-only launch gives the same bytes
    assert np.array_equal(interpret.decode_capsules(net, torch.from_numpy(t).cuda(), u8=True).cpu().numpy(), u8)


@pytest.mark.parametrize('N,C,labels', [(3, 43, [0, 42, 17]), (2, 5, [4, 0])])
def test_sweep_is_the_decode_of_the_host_built_vectors(net, N, C, labels):
    caps = wave((N, C, 16), 0.7, amp=0.4, freq=0.613)
    sweep = interpret.perturb_sweep(net, torch.from_numpy(caps).cuda(), np.array(labels), u8=False)
    assert sweep.shape == (N, 16, 11, 3, 32, 32) and sweep.dtype == torch.float32
    rows = np.zeros((N, 16, 11, 16), dtype=np.float32)
    for b in range(N):
        for v in range(16):
            for i in range(11):
                t = caps[b, labels[b]].copy()
                t[v] = t[v] + np.float32(interpret.DELTAS[i])
                rows[b, v, i] = t
    dense = interpret.decode_capsules(net, torch.from_numpy(rows.reshape(-1, 16)).cuda())
    assert torch.equal(dense, sweep.reshape(-1, 3, 32, 32))                       # bit for bit
    assert not torch.equal(sweep[:, :, 0], sweep[:, :, 10])
    u8 = interpret.perturb_sweep(net, torch.from_numpy(caps).cuda(), torch.tensor(labels).cuda())
    assert u8.shape == (N, 16, 11, 32, 32, 3) and u8.dtype == torch.uint8
    assert torch.equal(u8.reshape(-1, 32, 32, 3), interpret.decode_capsules(net, torch.from_numpy(rows.reshape(-1, 16)).cuda(), u8=True))


def test_sweep_column_of_delta_zero_is_reconstruct(net, params):
    x = synth.images(3, 32, seed=5)                                               # NHWC
    y = np.array([0, 42, 17])
    recon, sqerr = interpret.reconstruct(net, x, y, params)
    assert recon.shape == (3, 3, 32, 32) and sqerr.shape == (3,) and recon.is_cuda and sqerr.is_cuda
    with torch.no_grad():
        caps = net.capsules(torch.from_numpy(x).cuda().permute(0, 3, 1, 2).contiguous())
    assert caps.shape == (3, 43, 16)
    sweep = interpret.perturb_sweep(net, caps, y, u8=False)
    assert interpret.DELTAS[5] == 0
    for v in range(16):
        assert torch.equal(sweep[:, v, 5], recon)
    chunked, sq2 = interpret.reconstruct(net, x, y, params, batch_size=2)         # chunks of 2 + 1
    assert chunked.shape == recon.shape and sq2.shape == sqerr.shape


def test_through_the_model_against_the_fixture(net, oracle, params):
    g = load_golden('interpret')
    x = synth_images(3, 32, 7, nchw=False)
    labels = [int(v) for v in g['labels']]
    with torch.no_grad():
        caps = net.capsules(torch.from_numpy(x).cuda().permute(0, 3, 1, 2).contiguous()).cpu().numpy()
    np.testing.assert_allclose(caps, g['caps'], rtol=1e-4, atol=1e-5)             # the routing tolerance of test_gpu_kernels.py
    pick = g['digest_pick']
    loop = float(g['loop_to_clean64'])
    dig64 = np.concatenate([g['dig64_sums'], g['dig32_samples'].astype(np.float64) + g['dig64_minus_dig32']], axis=-1)
    dig32 = np.concatenate([g['dig32_sums'], g['dig32_samples'].astype(np.float64)], axis=-1)
    for b in range(3):
        res = interpret.interpret_sample(net, x[b], labels[b], params, u8=False)
        sweep = res['sweep'].cpu().numpy()
        assert sweep.shape == (16, 11, 3, 32, 32) and res['label'] == labels[b]
        # d32 of this sample's 176 vectors, by the oracle on the vectors the kernel was given
        rows = np.repeat(res['caps'].cpu().numpy()[labels[b]][None], 176, 0).reshape(16, 11, 16)
        for v in range(16):
            rows[v, :, v] += g['deltas']
        o32, o64 = _oracle_decode(oracle, rows.reshape(176, 16))
        d32 = float(np.abs(o32 - o64).max())
        tol = _tol(d32)
        got = np.array([[grad_digest(torch.from_numpy(sweep[v, i][None]))[pick] for i in range(11)] for v in range(16)])
        e64, e32 = np.abs(got - dig64[b]), np.abs(got - dig32[b])
        print('sample %d: d32 %.3g; samples off fp64 by %.3g (bound %.3g), off the fp32 loop by %.3g (bound %.3g); sums off by %.3g'
              % (b, d32, e64[..., 2:].max(), tol, e32[..., 2:].max(), tol + loop, e64[..., :2].max()))
        assert e64[..., 2:].max() <= tol and e32[..., 2:].max() <= tol + loop
        assert e64[..., :2].max() <= 3072 * tol and e32[..., :2].max() <= 3072 * (tol + loop)   # sums of 3 072 elements
        assert np.abs(sweep.reshape(176, 3, 32, 32).astype(np.float64) - o64).max() <= tol
        if b == 0:
            for k, (v, i) in enumerate(g['full_vi']):
                assert np.abs(sweep[v, i].astype(np.float64) - g['full32'][k]).max() <= tol + loop
        rel = abs(res['sqerr'] - float(g['sqerr64'][b])) / float(g['sqerr64'][b])
        print('sample %d: sqerr %.6f, fixture %.6f (relative %.3g; held to a bound by the sqerr test)'
              % (b, res['sqerr'], float(g['sqerr64'][b]), rel))


def test_sqerr_against_fp64_and_bit_identical(net, oracle, params):
    x = synth.images(5, 32, seed=9)
    y = np.array([1, 0, 42, 7, 30])
    recon, sqerr = interpret.reconstruct(net, x, y, params)
    recon2, sqerr2 = interpret.reconstruct(net, x, y, params)
    assert torch.equal(sqerr, sqerr2) and torch.equal(recon, recon2)              # two calls: identical bits
    with torch.no_grad():
        caps = net.capsules(torch.from_numpy(x).cuda().permute(0, 3, 1, 2).contiguous()).cpu().numpy()
    t = caps[np.arange(5), y]
    o32, o64 = oracle
    xn = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
    with torch.no_grad():
        s32 = ((xn - o32.decoder(torch.from_numpy(t))) ** 2).sum(dim=(1, 2, 3)).double().numpy()
        s64 = ((xn.double() - o64.decoder(torch.from_numpy(t).double())) ** 2).sum(dim=(1, 2, 3)).numpy()
    d32 = float(np.abs(s32 - s64).max() / s64.min())
    rel = np.abs(sqerr.cpu().numpy().astype(np.float64) - s64) / s64
    print('sqerr: d32 (relative) %.3g, kernel vs fp64 (relative) %.3g (bound %.3g)' % (d32, rel.max(), _tol(d32)))
    assert rel.max() <= _tol(d32)


def test_per_layer_path_and_fused_kernel_agree_with_fp64(net, dense):
    t, o32, o64 = (a[:37] for a in dense)
    tol = _tol(float(np.abs(o32 - o64).max()))
    td = torch.from_numpy(t).cuda()
    with torch.no_grad():
        layered = net.decoder(td).cpu().numpy().astype(np.float64)
    fused = interpret.decode_capsules(net, td).cpu().numpy().astype(np.float64)
    print('per-layer path vs fp64 %.3g, fused kernel vs fp64 %.3g (bound %.3g)'
          % (np.abs(layered - o64).max(), np.abs(fused - o64).max(), tol))
    assert np.abs(layered - o64).max() <= tol and np.abs(fused - o64).max() <= tol


def test_errors(net, params):
    with pytest.raises(_lib.HipExtensionError):
        interpret.decode_capsules(net, torch.zeros(4, 16))                        # a CPU tensor
    with pytest.raises(ValueError):
        interpret.decode_capsules(net, torch.zeros(4, 15, device='cuda'))
    caps = torch.from_numpy(wave((2, 5, 16), 0.1, amp=0.3)).cuda()
    with pytest.raises(ValueError, match='label'):
        interpret.perturb_sweep(net, caps, np.array([1, 5]))                      # a label equal to C
    with pytest.raises(ValueError, match='label'):
        interpret.perturb_sweep(net, caps, np.array([-1, 2]))
    empty = interpret.decode_capsules(net, torch.zeros(0, 16, device='cuda'))
    assert empty.shape == (0, 3, 32, 32) and empty.dtype == torch.float32
    assert interpret.decode_capsules(net, torch.zeros(0, 16, device='cuda'), u8=True).shape == (0, 32, 32, 3)
    _lib.TRACE = []
    try:
        interpret.decode_capsules(net, torch.zeros(0, 16, device='cuda'))
        assert _lib.TRACE == []                                                   # n = 0: no launch
        good = interpret.perturb_sweep(net, caps, np.array([1, 4]))               # ... and ONE launch for all N * 16 * 11 rows
        assert _lib.TRACE == ['cy_decoder_fwd'] and good.shape == (2, 16, 11, 32, 32, 3)
    finally:
        _lib.TRACE = None


def test_main_interpret_mode(tmp_path):
    cp = make_params(model='capsule', n_classes=43, device='cuda', batch_size=16)
    torch.manual_seed(3)
    cdir = str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.CapsuleNet(cp).state_dict()}, False, cdir)
    json.dump(dict(batch_size=16, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_interpret', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    res = m.main(['--mode', 'interpret', '--model', 'capsule', '--synthetic', '4', '--index', '2', '--model_dir', cdir, '--restore', 'last'])
    img = os.path.join(cdir, 'img')
    names = ['orig.ppm', 'sheet.ppm'] + ['%d-%d.ppm' % (v, i) for v in range(16) for i in range(11)]
    assert sorted(os.listdir(img)) == sorted(names + ['sweep.npy'])
    sweep = np.load(os.path.join(img, 'sweep.npy'))
    assert sweep.shape == (16, 11, 32, 32, 3) and sweep.dtype == np.uint8
    # the API on the same checkpoint and sample
    x, y = synth.images(4, 32), synth.gtsrb_labels(4, 43)
    caps = models.CapsuleNet(cp).cuda()
    utils.load_checkpoint(os.path.join(cdir, 'last.pth.tar'), caps, cp)
    api = interpret.interpret_sample(caps, x[2], int(y[2]), cp)
    assert np.array_equal(api['sweep'].cpu().numpy(), sweep)
    assert res['label'] == api['label'] == int(y[2]) and res['pred'] == api['pred'] and res['sqerr'] == api['sqerr']
    plain = np.clip(np.rint(api['recon'].cpu().numpy() * np.float32(128.0) + np.float32(128.0)), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(interpret.read_ppm(os.path.join(img, '5-5.ppm')), plain)
    assert np.array_equal(interpret.read_ppm(os.path.join(img, '3-7.ppm')), sweep[3, 7])
    assert np.array_equal(interpret.read_ppm(os.path.join(img, 'orig.ppm')), interpret.to_bytes(x[2]))
    sheet = interpret.read_ppm(os.path.join(img, 'sheet.ppm'))
    assert sheet.shape == (16 * 32, 11 * 32, 3) and np.array_equal(sheet[3 * 32:4 * 32, 7 * 32:8 * 32], sweep[3, 7])
    with pytest.raises(SystemExit):
        m.main(['--mode', 'interpret', '--model', 'cnn', '--synthetic', '4', '--model_dir', cdir, '--restore', 'last'])

"""CPU tests of capsule interpretation: the oracle's CapsuleNet against what the reference produced (tests/golden/interpret.npz,
written by tests/golden/make_golden_interpret.py) -- the GPU tests compare the kernel with the oracle, this pins the oracle to the
reference --, the host side of capsyolo_amd.interpret, the new `--index` argument and the C-ABI's new symbol and struct."""
import copy
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import REPO, closed_form_state, grad_digest, load_golden, make_params, synth_images

from capsyolo_amd import _lib, interpret
from oracle import models as OM

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gold():
    return load_golden('interpret')


def test_fixture_holds_data_only_and_stays_small(gold):
    assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', 'interpret.npz')) < 300 * 1024
    assert list(gold['labels']) == [3, 17, 42] and gold['caps'].shape == (3, 43, 16) and gold['caps'].dtype == np.float32
    assert np.array_equal(gold['deltas'], interpret.DELTAS)
    assert gold['dig32_sums'].shape == gold['dig64_sums'].shape == (3, 16, 11, 2)
    assert gold['dig32_samples'].shape == gold['dig64_minus_dig32'].shape == (3, 16, 11, 32)
    assert gold['full32'].shape == (8, 3, 32, 32) and gold['full32'].dtype == np.float32
    assert {(0, 0), (0, 10), (15, 0), (15, 10)} <= {tuple(int(c) for c in vi) for vi in gold['full_vi']}
    # what the issue measured for these inputs
    assert np.abs(gold['caps']).max() <= 0.014 and float(gold['loop_to_clean64']) <= 2.1e-7 and float(gold['drift']) <= 2e-8


def test_oracle_reproduces_the_fixture(gold):
    """The oracle driven like capsule_interpret.py (in place, float32) against the reference's float32 digests, at float32
    resolution; its float64 copy on the clean vectors against the reference's float64 digests, within 4 x the fixture's own
    float32-to-float64 distance (sums of 3 072 elements: 3 072 x that)."""
    p = make_params(n_classes=43, device='cpu', model='capsule')
    o = OM.CapsuleNet(p)
    o.load_state_dict(closed_form_state(o))
    o.eval()
    o64 = copy.deepcopy(o).double()
    x = torch.from_numpy(synth_images(3, 32, 7))
    pick, deltas = gold['digest_pick'], gold['deltas']
    cc = np.arange(11) * 0.05 - 0.25
    d64 = 4.0 * float(gold['loop_to_clean64'])
    worst32, worst64 = 0.0, 0.0
    with torch.no_grad():
        caps = o.traffic_sign_capsules(o.primary_capsules(F.relu(o.conv1(x))))[:, 0, :, 0, :]
        np.testing.assert_allclose(caps.numpy(), gold['caps'], rtol=1e-4, atol=1e-5)       # the routing tolerance of test_gpu_kernels.py
        print('oracle capsules off the reference\'s by %.3g' % np.abs(caps.numpy() - gold['caps']).max())
        for b, label in enumerate(int(v) for v in gold['labels']):
            t = torch.from_numpy(gold['caps'][b, label]).clone()               # the reference's own vector: the decoder alone from here
            t0 = t.clone()
            for v in range(16):
                clean = t0.repeat(11, 1)
                clean[:, v] += torch.from_numpy(deltas)
                dec64 = o64.decoder(clean.double())
                for i, c in enumerate(cc):
                    t[v] = t[v] + c
                    dig = grad_digest(o.decoder(t))[pick]
                    t[v] = t[v] - c
                    ref32 = np.concatenate([gold['dig32_sums'][b, v, i], gold['dig32_samples'][b, v, i].astype(np.float64)])
                    assert np.abs(dig[2:] - ref32[2:]).max() <= EPS32 and np.abs(dig[:2] - ref32[:2]).max() <= 3072 * EPS32
                    worst32 = max(worst32, float(np.abs(dig - ref32).max()))
                    dig = grad_digest(dec64[i:i + 1])[pick]
                    ref64 = np.concatenate([gold['dig64_sums'][b, v, i], ref32[2:] + gold['dig64_minus_dig32'][b, v, i]])
                    assert np.abs(dig[2:] - ref64[2:]).max() <= d64 and np.abs(dig[:2] - ref64[:2]).max() <= 3072 * d64
                    worst64 = max(worst64, float(np.abs(dig - ref64).max()))
                    if b == 0 and [v, i] in gold['full_vi'].tolist():
                        k = gold['full_vi'].tolist().index([v, i])
                        assert np.abs(dec64[i].numpy() - gold['full32'][k]).max() <= float(gold['loop_to_clean64']) + 1e-12
            s64 = float(((x[b:b + 1].double() - o64.decoder(t0.double())) ** 2).sum())
            assert abs(s64 - float(gold['sqerr64'][b])) <= 1e-9 * s64
    print('oracle vs fixture: float32 digests off by %.3g, float64 digests off by %.3g' % (worst32, worst64))


def test_deltas():
    assert interpret.DELTAS.dtype == np.float32 and interpret.DELTAS.shape == (11,)
    assert interpret.DELTAS[5] == 0 and interpret.DELTAS[0] == np.float32(-0.25) and interpret.DELTAS[10] == np.float32(0.25)
    assert np.array_equal(interpret.DELTAS, (np.arange(11) * 0.05 - 0.25).astype(np.float32))


def test_write_ppm_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)                # BGR, height 5, width 7
    path = str(tmp_path / 'a.ppm')
    interpret.write_ppm(path, img)
    raw = open(path, 'rb').read()
    assert raw.startswith(b'P6\n7 5\n255\n') and len(raw) == len(b'P6\n7 5\n255\n') + 5 * 7 * 3
    body = np.frombuffer(raw[len(b'P6\n7 5\n255\n'):], dtype=np.uint8).reshape(5, 7, 3)
    assert np.array_equal(body, img[:, :, ::-1])                         # the file holds RGB
    assert np.array_equal(interpret.read_ppm(path), img)
    with pytest.raises(ValueError):
        interpret.write_ppm(path, img.astype(np.float32))
    with pytest.raises(ValueError):
        interpret.write_ppm(path, img[:, :, :2])
    sheet = interpret.contact_sheet(rng.integers(0, 256, (16, 11, 4, 6, 3), dtype=np.uint8))
    assert sheet.shape == (64, 66, 3)
    x = np.array([[-1.0, -0.99609375, 0.0, 0.00390625, 0.01171875, 0.9921875, 1.0]], dtype=np.float32)
    assert interpret.to_bytes(x).tolist() == [[0, 0, 128, 128, 130, 255, 255]]     # 128.5 -> 128 and 129.5 -> 130: half to even; 256 -> 255


def test_host_side_refusals_need_no_gpu():
    with pytest.raises(_lib.HipExtensionError):
        interpret.decode_capsules(None, torch.zeros(4, 16))                # a CPU tensor: there is no CPU fallback
    with pytest.raises(_lib.HipExtensionError):
        interpret.perturb_sweep(None, torch.zeros(2, 5, 16), np.array([0, 1]))
    src = open(os.path.join(REPO, 'cs231-capsule-yolo-traffic-sign-detection_amd', 'interpret.py')).read()
    assert not re.search(r'^\s*(from|import)\s+oracle', src, re.M)         # the product does not import the oracle


def test_parser_knows_index():
    spec = importlib.util.spec_from_file_location('cy_main_interpret_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.parser.parse_args([]).index == 0
    a = m.parser.parse_args(['--mode', 'interpret', '--model', 'capsule', '--index', '7', '--restore', 'best'])
    assert a.index == 7 and a.mode == 'interpret'
    assert callable(m.interpret)


def test_cabi_declares_and_binds_the_decoder():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    assert re.search(r'\bcy_decoder_fwd\s*\(', header)
    assert 'cy_decoder_fwd' in _lib.EXPORTS and hasattr(lib, 'cy_decoder_fwd')
    assert len(_lib._SIGS['cy_decoder_fwd']) == 2
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6


def test_decoder_struct_matches_header_field_order():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    body = re.search(r'typedef struct \{([^{}]*)\}\s*cy_decoder_t;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(',')
        fields.append(names[0].split()[-1].lstrip('*'))
        fields.extend(n.strip().lstrip('*') for n in names[1:])
    assert fields == [f[0] for f in _lib.Decoder._fields_]
    import ctypes as C
    assert C.sizeof(_lib.Decoder) == 18 * 8 + 4 * 4                        # 18 pointers, 4 ints, no padding


def test_decoder_entry_point_validates_on_the_host():
    """Rejected by the argument check, before any launch: the pointers are never followed."""
    import ctypes as C
    ok = dict(caps=16, lin_w=16, lin_b=16, w4=16, b4=16, w7=16, b7=16, w10=16, b10=16, w12=16, b12=16, out_f32=16, n=4, C=1, D=16)
    for change, match in ((dict(caps=None), 'null'), (dict(w10=None), 'null'), (dict(n=0), 'n = 0'), (dict(C=0), 'C = 0'),
                          (dict(D=15), '15 floats'), (dict(out_f32=None), 'no output'), (dict(sqerr=16), 'sqerr needs'),
                          (dict(labels=16, C=43), 'error word'), (dict(deltas=16), 'deltas'), (dict(n_delta=3), 'deltas'),
                          (dict(n=1 << 30, deltas=16, n_delta=11), 'too many')):
        a = _lib.Decoder(**dict(ok, **change))
        with pytest.raises(_lib.HipExtensionError, match=match):
            _lib.call('cy_decoder_fwd', C.byref(a), None)
    with pytest.raises(_lib.HipExtensionError, match='null'):
        _lib.call('cy_decoder_fwd', None, None)

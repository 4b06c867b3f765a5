"""CPU tests of the NV12 path (csrc/crop_pixel.h, csrc/nv12.hip, capsyolo_amd/nv12.py, serve.SignDetector(frame_format='nv12')):
the colour rule's known answers and range, the layout, the host encoder, the exports, and every refusal that comes before any
device work."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO

import nv12_ref as R
from capsyolo_amd import _lib, nv12, serve

NAMES = {'cy_crop_resize_nv12': 17, 'cy_boxes_crop_resize_nv12': 19, 'cy_nv12_to_rgb_u8': 11}


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize('yuv,rgb,pre', [((16, 128, 128), (0, 0, 0), None), ((235, 128, 128), (255, 255, 255), None),
                                         ((0, 0, 0), (0, 154, 0), (-204, 154, -258)), ((255, 255, 255), (255, 125, 255), (481, 125, 534)),
                                         ((81, 90, 240), (254, 0, 0), (254, -1, -1)), ((145, 54, 34), (0, 255, 1), None)])
def test_known_answers_under_bt601(yuv, rgb, pre):
    assert tuple(int(v) for v in R.convert(*yuv)) == rgb
    got = tuple(int(v) for v in R.before_clamp(*yuv)[0])
    if pre is not None:
        assert got == pre
    if yuv == (145, 54, 34):
        assert got[1] == 256
    frame = np.array([yuv[0], 0x33, yuv[1], yuv[2]], dtype=np.uint8)             # 1 x 1, pitch 2: the byte behind Y belongs to no pixel
    assert R.to_rgb(frame, 1, 1).reshape(3).tolist() == list(rgb)


def test_tables_are_the_literals_of_the_rule():
    want = {'bt601': (16, 1220542, 1673527, 409993, 852492, 2116026), 'bt709': (16, 1220945, 1879825, 223607, 558796, 2215014),
            'bt601_full': (0, 1048576, 1470104, 360853, 748826, 1858077), 'bt709_full': (0, 1048576, 1651297, 196424, 490864, 1945738)}
    assert {k: tuple(v) for k, v in nv12.MATRICES.items()} == want == R.MATRICES
    assert nv12.coef('bt601') == nv12.MATRICES['bt601'] and nv12.coef() == nv12.MATRICES['bt601']
    assert nv12.coef((0, 1, 2, 3, 4, 5)) == nv12.YuvMatrix(0, 1, 2, 3, 4, 5) and nv12.YuvMatrix._fields == ('y_off', 'cy', 'cvr', 'cug', 'cvg', 'cub')
    c = nv12.c_coef('bt709')
    assert (c.y_off, c.cy, c.cvr, c.cug, c.cvg, c.cub) == want['bt709']
    for bad in ('bt2020', (1, 2, 3), (0, 1.5, 2, 3, 4, 5), (256, 1, 2, 3, 4, 5), (-1, 1, 2, 3, 4, 5), (16, 1 << 30, 0, 0, 0, 0),
                (16, 1220542, 1 << 25, 0, 0, 0), None, 7):
        with pytest.raises(ValueError):
            nv12.coef(bad)


@pytest.mark.parametrize('name', sorted(R.MATRICES))
def test_every_triple_stays_inside_int32(name):
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    worst, negative, over = 0, 0, 0
    for y in range(256):
        pre, big = R.before_clamp(np.full_like(u, y), u, v, name)
        worst = max(worst, big)
        negative += int((pre < 0).any(axis=-1).sum())
        over += int((pre > 255).any(axis=-1).sum())
    print('%s: largest magnitude in front of the shift %d, %.1f %% of the triples negative, %.1f %% over 255 in some channel'
          % (name, worst, 100.0 * negative / 2 ** 24, 100.0 * over / 2 ** 24))
    assert worst <= 5.93e8 < 2 ** 31 - 1
    assert negative > 0 and over > 0
    if name == 'bt601':
        assert round(100.0 * negative / 2 ** 24) == 46          # a truncating division would give other bytes on these


def test_chroma_index_comes_from_the_frame_coordinate():
    H, W, pitch = 7, 9, 13
    uv_off = H * pitch + 5
    assert R.nbytes(H, W, pitch, uv_off) == uv_off + 4 * pitch
    buf = np.arange(R.nbytes(H, W, pitch, uv_off), dtype=np.int64)             # every byte holds its own index (mod 256 below)
    Y, U, V = R.planes((buf % 251).astype(np.uint8), H, W, pitch, uv_off)
    for y, x in ((0, 0), (1, 1), (6, 8), (5, 8), (6, 7), (3, 4), (2, 5)):
        iy, iu = R.sample_index(y, x, pitch, uv_off)
        assert iy == y * pitch + x and iu == uv_off + (y // 2) * pitch + 2 * (x // 2)
        assert (Y[y, x], U[y, x], V[y, x]) == (iy % 251, iu % 251, (iu + 1) % 251)
    assert (U[6, 8], V[6, 8]) == ((uv_off + 3 * pitch + 8) % 251, (uv_off + 3 * pitch + 9) % 251)    # the last, half-empty block
    assert (U[0::2, 0::2][:3, :4] == U[1::2, 1::2]).all() and (V[0::2, 0::2][:3, :4] == V[1::2, 1::2]).all()   # one pair per 2 x 2
    lay = nv12.Layout(H, W, pitch, uv_off)
    assert lay.nbytes == R.nbytes(H, W, pitch, uv_off) and lay.geom == (H, W, pitch, uv_off)


def test_layout_defaults_and_validation():
    lay = nv12.Layout(7, 9)
    assert (lay.pitch, lay.uv_off, lay.nbytes) == (10, 70, 70 + 4 * 10) == R.tight(7, 9) + (R.nbytes(7, 9),)
    assert nv12.Layout(8, 10) == nv12.Layout(8, 10, 10, 80) and hash(nv12.Layout(8, 10)) == hash(nv12.Layout(8, 10, 10, 80))
    assert nv12.Layout(8, 10) != nv12.Layout(8, 10, 16) and len({nv12.Layout(8, 10), nv12.Layout(8, 10, 16)}) == 2
    assert nv12.Layout(1, 1).nbytes == 4 and nv12.Layout(2, 2).nbytes == 6
    with pytest.raises(ValueError, match='pitch'):
        nv12.Layout(7, 9, pitch=9)                      # 1: pitch >= 2 ceil(W / 2)
    with pytest.raises(ValueError, match='uv_off'):
        nv12.Layout(7, 9, pitch=10, uv_off=69)          # 2: uv_off >= H pitch
    with pytest.raises(ValueError, match='does not lie inside'):
        lay.check(-1, 1000)                             # 3: img_off >= 0
    with pytest.raises(ValueError, match='does not lie inside'):
        lay.check(5, 5 + lay.nbytes - 1)                # 4: the end of the chroma plane inside the buffer
    lay.check(5, 5 + lay.nbytes)
    for bad in ((0, 4), (4, 0), (4.5, 4), (True, 4)):
        with pytest.raises(ValueError):
            nv12.Layout(*bad)
    with pytest.raises(AttributeError):
        lay.pitch = 12
    assert nv12.Layout.of(np.zeros((12, 10), np.uint8)) == nv12.Layout(8, 10)
    for shape in ((12, 9), (11, 10), (12, 10, 3), (12,)):
        with pytest.raises(ValueError):
            nv12.Layout.of(np.zeros(shape, np.uint8))


def test_from_rgb_grey_padding_and_round_trip():
    for m in sorted(nv12.MATRICES):
        for g in (0, 16, 77, 128, 235, 255):
            f = nv12.from_rgb(np.full((6, 8, 3), g, np.uint8), m)
            assert f.shape == (9, 8) and (f[6:] == 128).all(), (m, g)
            back = R.to_rgb(f, matrix=m).astype(np.int64)
            assert np.abs(back - g).max() <= 1, (m, g)
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    lay = nv12.Layout(7, 9, pitch=16, uv_off=7 * 16 + 32)
    padded = nv12.from_rgb(rgb, 'bt601', lay)
    tight = nv12.from_rgb(rgb, 'bt601')
    assert padded.shape == (lay.nbytes,) and tight.shape == (nv12.Layout(7, 9).nbytes,)
    assert nv12.PAD not in (0, 128)
    owned = np.zeros(lay.nbytes, bool)
    for y in range(7):
        for x in range(9):
            iy, iu = R.sample_index(y, x, lay.pitch, lay.uv_off)
            owned[[iy, iu, iu + 1]] = True
    assert (padded[~owned] == nv12.PAD).all() and owned.sum() == 7 * 9 + 4 * 10
    want = R.to_rgb(padded, 7, 9, lay.pitch, lay.uv_off)
    np.testing.assert_array_equal(want, R.to_rgb(tight, 7, 9))                   # the same samples in both layouts
    scribbled = padded.copy()
    scribbled[~owned] = rng.integers(0, 256, int((~owned).sum()), dtype=np.uint8)
    np.testing.assert_array_equal(R.to_rgb(scribbled, 7, 9, lay.pitch, lay.uv_off), want)     # to_rgb reads no padding byte
    # the luma of a smooth image survives the trip (chroma is subsampled: only Y is compared, through grey)
    ramp = np.repeat(np.arange(0, 256, 4, dtype=np.uint8).reshape(8, 8, 1), 3, axis=2)
    assert np.abs(R.to_rgb(nv12.from_rgb(ramp)).astype(np.int64) - ramp).max() <= 1
    with pytest.raises(ValueError):
        nv12.from_rgb(rgb, 'bt601', nv12.Layout(8, 10))
    with pytest.raises(ValueError):
        nv12.from_rgb(rgb.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name, argc in NAMES.items():
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m and len(m.group(1).split(',')) == argc, name
        assert name in _lib.EXPORTS and hasattr(lib, name) and len(_lib._SIGS[name]) == argc
        assert _lib._SIGS[name][5] is _lib.YuvCoef
    assert re.search(r'typedef struct \{ int y_off, cy, cvr, cug, cvg, cub; \} cy_yuv_coef_t;', header)
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6


BT601 = _lib.YuvCoef(*R.MATRICES['bt601'])
WIDE = _lib.YuvCoef(16, 1 << 30, 0, 0, 0, 0)


def _resize_args(**kw):
    a = dict(imgs=8, img_off=8, img_geom=8, n_images=1, imgs_bytes=48, coef=BT601, box_img=8, rect=8, n=2, OH=8, OW=8, shift=0.0, scale=1.0,
             to_nchw=1, out=8, err=8)
    a.update(kw)
    return [a[k] for k in ('imgs', 'img_off', 'img_geom', 'n_images', 'imgs_bytes', 'coef', 'box_img', 'rect', 'n', 'OH', 'OW', 'shift',
                           'scale', 'to_nchw', 'out', 'err')] + [None]


@pytest.mark.parametrize('kw,msg', [(dict(imgs=None), 'null argument'), (dict(img_geom=None), 'null argument'), (dict(err=None), 'null argument'),
                                    (dict(n_images=0), 'bad sizes'), (dict(n=0), 'bad sizes'), (dict(OH=0), 'bad sizes'),
                                    (dict(OW=1 << 20), 'bad sizes'), (dict(imgs_bytes=0), 'bad sizes'), (dict(coef=WIDE), 'inside int32'),
                                    (dict(coef=_lib.YuvCoef(300, 1, 1, 1, 1, 1)), 'y_off must be in 0..255'),
                                    (dict(n=1 << 30, OH=1 << 10, OW=1 << 10), 'too many for one launch')])
def test_resize_entry_point_refuses_bad_arguments(kw, msg):
    with pytest.raises(_lib.HipExtensionError, match='cy_crop_resize_nv12: .*' + re.escape(msg)):
        _lib.call('cy_crop_resize_nv12', *_resize_args(**kw))


def _boxes_args(**kw):
    a = dict(imgs=8, img_off=8, img_geom=8, n_images=1, imgs_bytes=48, coef=BT601, count=8, box_img=8, box_xy=8, K=4, OH=8, OW=8, shift=0.0,
             scale=1.0, to_nchw=1, out=8, rect_out=8, err=8)
    a.update(kw)
    return [a[k] for k in ('imgs', 'img_off', 'img_geom', 'n_images', 'imgs_bytes', 'coef', 'count', 'box_img', 'box_xy', 'K', 'OH', 'OW',
                           'shift', 'scale', 'to_nchw', 'out', 'rect_out', 'err')] + [None]


@pytest.mark.parametrize('kw,msg', [(dict(count=None), 'null argument'), (dict(out=None), 'null argument'),
                                    (dict(rect_out=None), 'null argument'), (dict(err=None), 'null argument'),
                                    (dict(K=-1), 'K=-1'), (dict(OH=0), 'output size 0 x 8'), (dict(OW=-3), 'output size 8 x -3'),
                                    (dict(box_xy=None), 'null argument'), (dict(imgs=None), 'null argument'),
                                    (dict(img_geom=None), 'null argument'), (dict(n_images=0), '0 images'), (dict(coef=WIDE), 'inside int32'),
                                    (dict(K=1 << 20, OH=1 << 19, OW=1 << 19), 'too many for one launch')])
def test_boxes_entry_point_refuses_bad_arguments(kw, msg):
    with pytest.raises(_lib.HipExtensionError, match='cy_boxes_crop_resize_nv12: .*' + re.escape(msg)):
        _lib.call('cy_boxes_crop_resize_nv12', *_boxes_args(**kw))


def test_boxes_entry_point_with_no_slots_is_a_no_op():
    _lib.call('cy_boxes_crop_resize_nv12', *_boxes_args(K=0, imgs=None, box_img=None, box_xy=None))      # nothing is launched


@pytest.mark.parametrize('kw,msg', [(dict(imgs=None), 'null argument'), (dict(out=None), 'null argument'), (dict(out_off=None), 'null argument'),
                                    (dict(err=None), 'null argument'), (dict(n_images=0), '0 images'), (dict(n_images=65536), '65536 images'),
                                    (dict(imgs_bytes=0), 'in 0 bytes'), (dict(out_bytes=0), 'to 0 bytes'), (dict(coef=WIDE), 'inside int32')])
def test_to_rgb_entry_point_refuses_bad_arguments(kw, msg):
    a = dict(imgs=8, img_off=8, img_geom=8, n_images=1, imgs_bytes=48, coef=BT601, out=8, out_off=8, out_bytes=96, err=8)
    a.update(kw)
    with pytest.raises(_lib.HipExtensionError, match='cy_nv12_to_rgb_u8: .*' + re.escape(msg)):
        _lib.call('cy_nv12_to_rgb_u8', *([a[k] for k in ('imgs', 'img_off', 'img_geom', 'n_images', 'imgs_bytes', 'coef', 'out', 'out_off',
                                                          'out_bytes', 'err')] + [None]))


# ------------------------------------------------------------------------------------------------ SignDetector and the command line
def test_sign_detector_refuses_bad_format_arguments_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(ValueError, match='frame_format'):
        serve.SignDetector(None, None, None, None, frame_format='yuv')
    with pytest.raises(ValueError, match="yuv_matrix belongs to frame_format='nv12'"):
        serve.SignDetector(None, None, None, None, yuv_matrix='bt709')
    with pytest.raises(ValueError, match="yuv_matrix belongs to frame_format='nv12'"):
        serve.SignDetector(None, None, None, None, frame_format='rgb', yuv_matrix=nv12.MATRICES['bt601'])
    with pytest.raises(ValueError, match='bt2020'):
        serve.SignDetector(None, None, None, None, frame_format='nv12', yuv_matrix='bt2020')
    with pytest.raises(ValueError, match='six integers'):
        serve.SignDetector(None, None, None, None, frame_format='nv12', yuv_matrix=(1, 2, 3))
    for kw in (dict(frame_format='nv12'), dict(frame_format='nv12', yuv_matrix=(16, 1220542, 1673527, 409993, 852492, 2116026)), dict()):
        with pytest.raises(_lib.HipExtensionError, match='no CPU path'):          # the arguments pass; the GPU is what is missing
            serve.SignDetector(None, None, None, None, **kw)


def _main():
    spec = importlib.util.spec_from_file_location('cy_main_nv12_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_arguments_and_refusals():
    m = _main()
    d = m.parser.parse_args([])
    assert (d.frame_format, d.yuv_matrix, d.device_frames) == ('rgb', None, False)
    base = ['--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last']
    a = m.parser.parse_args(['--mode', 'serve'] + base + ['--frame_format', 'nv12', '--yuv_matrix', 'bt709', '--device_frames'])
    assert (a.frame_format, a.yuv_matrix, a.device_frames) == ('nv12', 'bt709', True)
    m.check_frames(a)
    m.check_frames(m.parser.parse_args(['--mode', 'serve'] + base + ['--device_frames']))         # packed RGB frames on the device
    for argv in (['--mode', 'predict'] + base + ['--frame_format', 'nv12'],
                 ['--mode', 'detect', '--model', 'darknet_d', '--restore', 'last', '--device_frames'],
                 ['--mode', 'serve'] + base + ['--yuv_matrix', 'bt709'],
                 ['--mode', 'serve'] + base + ['--frame_format', 'nv12', '--yuv_matrix', 'bt2020'],
                 ['--mode', 'train', '--model', 'capsule', '--yuv_matrix', 'bt601']):
        with pytest.raises(SystemExit):
            m.main(argv)
    odd = np.zeros((7, 9, 3), np.uint8)
    assert m.even_frame(odd).shape == (6, 8, 3) and m.even_frame(odd[:6, :8]).shape == (6, 8, 3)

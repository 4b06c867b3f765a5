"""GPU tests of the streaming detector (csrc/serve.hip behind capsyolo_amd/serve.py, `main.py --mode serve`).  The yardsticks: the
existing two-stage chain (PackedImages.crop_resize, utils.decode_boxes_device, utils.crop_rectangles, the models' eval forwards), bit
for bit, and the numpy restatements of tests/serve_ref.py for the rectangle policy and the record packing."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, make_params

import serve_ref as R
from capsyolo_amd import models, predict_fns, serve, synth, utils
from capsyolo_amd._lib import call

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


# ------------------------------------------------------------------------------------------------ the crop kernel
CROP_HW = [(12, 10), (9, 17)]
CROP_IDX = np.array([0, 1, 0, 1, 0, 1, 0, 1])
CROP_XY = np.array([[2.3, 3.7, 7.9, 9.2],          # interior
                    [-3.5, -2.2, 6.8, 5.1],        # hangs over the left / top border: clipped
                    [6.1, 8.4, 25.0, 30.0],        # hangs over the right / bottom border
                    [16.2, 8.1, 17.9, 9.5],        # one pixel, the last of its image
                    [4.2, 5.0, 4.9, 8.0],          # empty after truncation
                    [1.0, np.nan, 5.0, 5.0],       # a corner that is not a number
                    [0.0, 0.0, 10.0, 12.0],        # slots 6 and 7 are live only when the count says so
                    [3.0, 2.0, 9.0, 7.0]])
CROP_BAD = [4, 5]


def _crop_images():
    rng = np.random.default_rng(17)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in CROP_HW]


def _boxes_crop(packed, count, idx, xy, K, side, shift, scale, to_nchw):
    words = _dev([count, 0], np.int32)
    out = torch.full((K, 3, side, side) if to_nchw else (K, side, side, 3), float('nan'), dtype=torch.float32, device='cuda')
    rect = torch.full((K, 4), -7, dtype=torch.int32, device='cuda')
    bi, bxy = _dev(idx, np.int32), _dev(xy, np.float64)
    call('cy_boxes_crop_resize_u8', packed.buf.data_ptr(), packed.off.data_ptr(), packed.hw32.data_ptr(), packed.n, packed.nbytes,
         words.data_ptr(), bi.data_ptr(), bxy.data_ptr(), K, side, side, float(shift), float(scale), int(to_nchw), out.data_ptr(),
         rect.data_ptr(), words.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy(), rect.cpu().numpy(), int(words[1].item())


@pytest.mark.parametrize('side', [5, 32])
@pytest.mark.parametrize('to_nchw', [False, True])
@pytest.mark.parametrize('shift,scale', [(0.0, 1.0), (-128.0, 1.0 / 128.0)])
def test_boxes_crop_equals_the_existing_path_bit_for_bit(side, to_nchw, shift, scale):
    packed = predict_fns.PackedImages(_crop_images())
    K = 8
    for count in (6, 20, 0):
        live = min(count, K)
        good = [s for s in range(live) if s not in CROP_BAD]
        out, rect, err = _boxes_crop(packed, count, CROP_IDX, CROP_XY, K, side, shift, scale, to_nchw)
        ref_rect, ref_bad, ref_live = R.slot_rectangles(count, CROP_IDX, CROP_XY, CROP_HW, K)
        assert np.array_equal(rect, ref_rect) and ref_live.sum() == live
        assert err == int(ref_bad.sum()) == len([s for s in CROP_BAD if s < live])
        if good:
            want_rect = utils.crop_rectangles(CROP_XY[good], CROP_IDX[good], packed.hw)
            assert np.array_equal(rect[good], want_rect)
            want = packed.crop_resize(CROP_IDX[good], want_rect, side, side, shift, scale, to_nchw).cpu().numpy()
            np.testing.assert_array_equal(out[good], want)
        rest = [s for s in range(K) if s not in good]                    # bad and dead slots: exactly zero, zero rectangle
        assert not out[rest].any() and not np.isnan(out).any() and not rect[rest].any()
    assert (rect == 0).all() and err == 0                                # the last pass: no live slot at all


def test_boxes_crop_takes_a_bad_image_index_as_a_bad_slot():
    packed = predict_fns.PackedImages(_crop_images())
    idx = np.array([0, 2, -1, 1])
    xy = np.array([[1.0, 1.0, 5.0, 5.0]] * 4)
    out, rect, err = _boxes_crop(packed, 4, idx, xy, 4, 8, 0.0, 1.0, True)
    assert err == 2 and rect.tolist() == [[1, 5, 1, 5], [0, 0, 0, 0], [0, 0, 0, 0], [1, 5, 1, 5]]
    assert not out[1:3].any() and out[0].any() and out[3].any()


# ------------------------------------------------------------------------------------------------ the pack kernel
@pytest.mark.parametrize('C', [3, 43])
@pytest.mark.parametrize('count', [9, 4, 0])
def test_pack_detections_against_the_restatement(C, count):
    K = 6
    rng = np.random.default_rng(100 + C)
    scores = rng.random((K, C), dtype=np.float32)
    scores[1, [0, C - 1]] = 2.0                                          # a tie: the first index wins
    scores[2, 1] = np.nan                                                # a NaN counts as the maximum
    scores[2, 2] = 5.0
    scores[4, C // 2] = 3.0
    rect = np.array([[1, 5, 1, 5], [0, 2, 0, 2], [3, 4, 3, 4], [0, 0, 0, 0], [2, 9, 1, 3], [0, 1, 0, 1]], dtype=np.int32)   # slot 3 is bad
    idx = rng.integers(0, 3, K).astype(np.int32)
    xy = rng.random((K, 4)) * 100.0
    conf = rng.random(K, dtype=np.float32)
    words = _dev([count, 1, 0], np.int32)
    record = torch.full((serve.record_bytes(K),), 0xAB, dtype=torch.uint8, device='cuda')
    d = [_dev(scores, np.float32), _dev(idx, np.int32), _dev(xy, np.float64), _dev(conf, np.float32), _dev(rect, np.int32)]
    call('cy_pack_detections', d[0].data_ptr(), C, words.data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
         words.data_ptr() + 4, words.data_ptr() + 8, K, record.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = record.cpu().numpy()
    np.testing.assert_array_equal(got, R.pack(scores, count, idx, xy, conf, rect, 1, 0, K))
    res = serve.Detections(got, K)
    assert res.total == count and res.n == min(count, K) and res.truncated == (count > K) and res.bad == {'boxes': 1, 'frames': 0}
    want_cls = [int(np.argmax(scores[s])) if s != 3 else -1 for s in range(res.n)]
    assert res.classes.tolist() == want_cls
    if count >= 4:
        assert want_cls[1] == 0 and want_cls[2] == 1 and np.isnan(res.class_scores[2]) and res.class_scores[3] == 0


# ------------------------------------------------------------------------------------------------ the pipeline
K_PIPE = 8


def _frames(seed, h=80, w=100, n=2):
    return [im[:h, :w] for im in synth.raw_images(n, seed=seed, min_side=max(h, w), max_side=160)]


class _Chain(object):
    """The models of every pipeline test, and the existing chain's answer for one frame pair at one threshold."""

    def __init__(self):
        self.dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
        self.cp = make_params(model='capsule', n_classes=3, device='cuda')
        torch.manual_seed(3)
        self.dark, self.caps = models.DarkNet(self.dp).cuda().eval(), models.CapsuleNet(self.cp).cuda().eval()
        self.frames = _frames(41)
        with torch.no_grad():
            y = self.forward(self.frames)
            conf = np.unique(y[..., 0::5].cpu().numpy())[::-1].astype(np.float64)
            print('confidences: %s' % conf)
            assert len(conf) >= 7, 'the detector output has too few distinct confidences: %s' % conf
            self.conf_th = float(conf[4] + conf[5]) / 2
            self.n, self.idx, self.xy, self.conf, self.crops = self.decode(self.frames, y, self.conf_th)

    def forward(self, frames):
        return self.dark(predict_fns.PackedImages(frames).resize(64, to_nchw=True)).data

    def decode(self, frames, y, conf_th):
        packed = predict_fns.PackedImages(frames)
        n, idx, xy, _, conf = utils.decode_boxes_device(y, self.dp, packed.hw, conf_th, with_conf=True)
        idx, xy, conf = idx.cpu().numpy().astype(np.int64), xy.cpu().numpy(), conf.cpu().numpy()
        crops = None
        if n:
            rect = utils.crop_rectangles(xy, idx, packed.hw)
            crops = packed.crop_resize(idx, rect, 32, 32, -128.0, 1.0 / 128.0, True)
        return n, idx, xy, conf, crops


@pytest.fixture(scope='module')
def chain():
    return _Chain()


def test_pipeline_equals_the_existing_chain(chain):
    n = chain.n
    assert 1 <= n <= K_PIPE - 1, 'precondition: conf_th %.6f lets %d boxes through' % (chain.conf_th, n)
    det = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=K_PIPE, conf_th=chain.conf_th)
    res = det.detect(chain.frames)
    assert (res.n, res.total, res.truncated, res.bad) == (n, n, False, {'boxes': 0, 'frames': 0})
    np.testing.assert_array_equal(res.image_indices, chain.idx)
    np.testing.assert_array_equal(res.boxes_xy, chain.xy)
    np.testing.assert_array_equal(res.conf, chain.conf)
    with torch.no_grad():
        padded = torch.cat([chain.crops, torch.zeros((K_PIPE - n, 3, 32, 32), dtype=torch.float32, device='cuda')])
        scores = chain.caps(padded).data.reshape(K_PIPE, -1).cpu().numpy()[:n]
        alone = chain.caps(chain.crops).data.reshape(n, -1).cpu().numpy()
    np.testing.assert_array_equal(res.classes, np.argmax(scores, axis=1))
    np.testing.assert_array_equal(res.class_scores, scores[np.arange(n), np.argmax(scores, axis=1)])
    top = np.sort(alone.astype(np.float64), axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-3
    print('%d boxes, %d with a clear arg-max in the un-padded batch' % (n, clear.sum()))
    assert clear.any() and np.array_equal(res.classes[clear], np.argmax(alone, axis=1)[clear])
    again = det.detect(np.stack(chain.frames))                           # an [n, H, W, 3] array; the same state
    np.testing.assert_array_equal(again.record, res.record)
    assert len(det.states) == 1


def test_overflow_and_empty(chain):
    with torch.no_grad():
        full = chain.decode(chain.frames, chain.forward(chain.frames), 0.0)
    assert full[0] == 16
    det = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=4, conf_th=0.0)
    res = det.detect(chain.frames)
    assert res.total == 16 and res.n == 4 and res.truncated
    np.testing.assert_array_equal(res.image_indices, full[1][:4])
    np.testing.assert_array_equal(res.boxes_xy, full[2][:4])
    np.testing.assert_array_equal(res.conf, full[3][:4])
    assert (res.classes >= 0).all() and res.bad['boxes'] == 0
    none = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=4, conf_th=1.0).detect(chain.frames)
    assert none.n == 0 and none.total == 0 and not none.truncated and none.bad == {'boxes': 0, 'frames': 0}
    assert none.image_indices.shape == (0,) and none.boxes_xy.shape == (0, 4) and none.classes.shape == (0,)
    assert none.conf.shape == (0,) and none.class_scores.shape == (0,)


def test_refusals_on_the_device(chain):
    det = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=4)
    with pytest.raises(ValueError, match='one size'):
        det.detect([chain.frames[0], chain.frames[1][:, :90]])
    with pytest.raises(ValueError, match='uint8'):
        det.detect(chain.frames[0].astype(np.float32))
    wrong = make_params(model='darknet_d', n_classes=9, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    with pytest.raises(ValueError, match='no box left'):               # 10 values per cell, 9 of them class scores
        serve.SignDetector(chain.dark, wrong, chain.caps, chain.cp, max_boxes=4).detect(chain.frames)


def test_graph_equals_eager(chain):
    eager = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=K_PIPE, conf_th=chain.conf_th)
    graphed = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=K_PIPE, conf_th=chain.conf_th, graph=True)
    records = []
    for seed in (41, 42, 43):
        frames = _frames(seed)
        a, b = eager.detect(frames), graphed.detect(frames)
        np.testing.assert_array_equal(b.record, a.record)
        records.append(a.record)
    assert not np.array_equal(records[0], records[1]) and len(graphed.states) == 1
    state = graphed.states[(2, 80, 100)]
    first_graph = state.graph
    assert first_graph is not None
    one = _frames(44, 64, 72, 1)                                         # another shape: a second state with its own capture
    np.testing.assert_array_equal(graphed.detect(one[0]).record, eager.detect(one[0]).record)
    assert sorted(graphed.states) == [(1, 64, 72), (2, 80, 100)] and state.graph is first_graph
    # new weights: the capture holds the folded eval weights of the old ones and must be rebuilt
    before = graphed.detect(chain.frames).record
    saved = [dict((k, v.clone()) for k, v in m.state_dict().items()) for m in (chain.dark, chain.caps)]
    try:
        torch.manual_seed(11)
        chain.dark.load_state_dict(models.DarkNet(chain.dp).state_dict())
        chain.caps.load_state_dict(models.CapsuleNet(chain.cp).state_dict())
        after = graphed.detect(chain.frames).record
        fresh = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=K_PIPE, conf_th=chain.conf_th)
        np.testing.assert_array_equal(after, fresh.detect(chain.frames).record)
        assert not np.array_equal(after, before) and state.graph is not first_graph
    finally:
        chain.dark.load_state_dict(saved[0])
        chain.caps.load_state_dict(saved[1])
    np.testing.assert_array_equal(graphed.detect(chain.frames).record, before)


def test_plain_torch_classifier(chain):
    cp = make_params(model='cnn', n_classes=3, dropout=0.0, device='cuda')
    torch.manual_seed(5)
    cnn = models.ConvNet(cp).cuda()
    eager = serve.SignDetector(chain.dark, chain.dp, cnn, cp, max_boxes=K_PIPE, conf_th=chain.conf_th)
    graphed = serve.SignDetector(chain.dark, chain.dp, cnn, cp, max_boxes=K_PIPE, conf_th=chain.conf_th, graph=True)
    a, b = eager.detect(chain.frames), graphed.detect(chain.frames)
    np.testing.assert_array_equal(b.record, a.record)
    np.testing.assert_array_equal(graphed.detect(chain.frames).record, a.record)       # a replay after the capturing call
    assert a.n == chain.n and (a.classes >= 0).all() and (a.classes < 3).all()
    np.testing.assert_array_equal(a.boxes_xy, chain.xy)


# ------------------------------------------------------------------------------------------------ the command line
def test_main_serve_mode(tmp_path):
    dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    cp = make_params(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(3)
    ddir, cdir = str(tmp_path / 'darknet_d'), str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.DarkNet(dp).state_dict()}, False, ddir)
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.CapsuleNet(cp).state_dict()}, False, cdir)
    json.dump(dict(batch_size=4, n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, dropout=0.0),
              open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_serve', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--synthetic', '3', '--graph', '--model_dir', ddir,
                  '--restore', 'last'])
    lines = open(os.path.join(ddir, 'serve_output.txt')).read().splitlines()
    assert len(lines) == 3 and [ln.split(':')[0] for ln in lines] == ['frame 0', 'frame 1', 'frame 2']
    assert out['frames'] == 3 and out['boxes'] == sum(int(ln.split('boxes: ')[1].split(' of ')[0]) for ln in lines)
    with pytest.raises(SystemExit):
        m.main(['--mode', 'serve', '--model', 'darknet_d', '--synthetic', '3', '--model_dir', ddir, '--restore', 'last'])
    with pytest.raises(SystemExit):
        m.main(['--mode', 'serve', '--model', 'capsule', '--combine', 'capsule', '--synthetic', '3', '--model_dir', cdir, '--restore', 'last'])

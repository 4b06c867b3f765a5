"""GPU tests of the suppression step (csrc/nms.hip behind utils.nms_boxes_device / nms_y_hat_device, the nms arguments of
predict_fns.dark_pred / dark_class_pred, serve.SignDetector and main.py).  The yardstick is the numpy restatement tests/nms_ref.py,
bit for bit: the kernel copies its inputs and decides on the shared double-precision IoU, so the keep mask, the count and every
output array must be equal, not close."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, make_params

import nms_ref as R
import serve_ref
from capsyolo_amd import models, predict_fns, serve, synth, utils
from capsyolo_amd._lib import call

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _run(img, xy, conf, cls, n_images, iou_th=0.45, class_aware=False, per_image=0, max_per_image=1024, K=None, count=None, n_cap=None):
    """One `cy_nms_boxes` call on buffers of n_cap entries (default: the list) prefilled with junk behind the list and in every output."""
    n = len(img)
    n_cap = n if n_cap is None else n_cap
    K = n if K is None else K
    count = n if count is None else count
    pad = max(n_cap - n, 0)
    d_img = _dev(np.concatenate([np.asarray(img, np.int32)[:n_cap], np.full(pad, 0, np.int32)]), np.int32)
    d_xy = _dev(np.concatenate([np.asarray(xy, np.float64).reshape(-1, 4)[:n_cap], np.full((pad, 4), 5.0)]), np.float64)
    d_conf = _dev(np.concatenate([np.asarray(conf, np.float32)[:n_cap], np.full(pad, 0.99, np.float32)]), np.float32)
    d_cls = _dev(np.concatenate([np.asarray(cls, np.int32)[:n_cap], np.zeros(pad, np.int32)]), np.int32) if cls is not None else None
    keep = torch.full((n_cap,), -7, dtype=torch.int32, device='cuda')
    o_img, o_src = (torch.full((K,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    o_cls = torch.full((K,), -7, dtype=torch.int32, device='cuda')
    o_xy = torch.full((K, 4), float('nan'), dtype=torch.float64, device='cuda')
    o_conf = torch.full((K,), float('nan'), dtype=torch.float32, device='cuda')
    words = _dev([count, -7, 0] + [-7] * n_images, np.int32)            # count_in, count_out, err, scratch
    w = words.data_ptr()
    call('cy_nms_boxes', w, d_img.data_ptr(), d_xy.data_ptr(), d_conf.data_ptr(), d_cls.data_ptr() if cls is not None else None, n_cap,
         n_images, float(iou_th), int(class_aware), per_image, max_per_image, keep.data_ptr(), K, o_img.data_ptr(), o_xy.data_ptr(),
         o_conf.data_ptr(), o_cls.data_ptr() if cls is not None else None, o_src.data_ptr(), w + 4, w + 12, w + 8,
         torch.cuda.current_stream().cuda_stream)
    wd = words.cpu().numpy()
    return dict(keep=keep.cpu().numpy(), count=int(wd[1]), err=int(wd[2]), img=o_img.cpu().numpy(), xy=o_xy.cpu().numpy(),
                conf=o_conf.cpu().numpy(), cls=o_cls.cpu().numpy() if cls is not None else None, src=o_src.cpu().numpy())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(got, img, xy, conf, cls, n_images, K=None, **kw):
    """got == the restatement, bit for bit: keep, count and the K slots of every output array."""
    n = len(img)
    K = n if K is None else K
    keep, order, visited, overflow = R.nms(img, xy, conf, cls, n_images=n_images, **kw)
    count, o_img, o_xy, o_conf, o_cls, o_src = R.outputs(order, img, xy, conf, cls, K)
    assert got['err'] == overflow << 20
    np.testing.assert_array_equal(got['keep'][:n], keep)
    assert got['count'] == count == int(keep.sum())
    assert _same_bits(got['img'], o_img) and _same_bits(got['src'], o_src)
    assert _same_bits(got['xy'], o_xy) and _same_bits(got['conf'], o_conf)        # bytes: a NaN corner is a copy too
    if cls is not None:
        assert _same_bits(got['cls'], o_cls)
    return keep, visited


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', sorted(R.known_answers()))
def test_known_answers(name):
    kw, want = R.known_answers()[name]
    kw = dict(kw)
    img, xy, conf, cls = kw.pop('box_img'), kw.pop('box_xy'), kw.pop('conf'), kw.pop('cls', None)
    n_images = kw.pop('n_images', max(img) + 1)
    got = _run(img, xy, conf, cls, n_images, **kw)
    assert got['keep'].tolist() == want
    _check(got, np.asarray(img), xy, conf, cls, n_images, **kw)


# 256 is the kernel's one internal size (positions per sweep step); 1025 boxes need more LDS than a launch gets without opting in
@pytest.mark.parametrize('counts', [(1, 0, 255), (256, 0, 257), (257, 0, 1), (513, 0, 2), (1025, 0, 3)])
@pytest.mark.parametrize('class_aware', [False, True])
def test_integer_corner_lists(counts, class_aware):
    img, xy, conf, cls = R.integer_lists(counts, seed=sum(counts))
    assert len(np.unique(conf)) < len(conf) / 2 or len(conf) < 300      # confidence ties are there
    kw = dict(iou_th=0.45, class_aware=class_aware)
    got = _run(img, xy, conf, cls, 3, max_per_image=max(counts), **kw)
    keep, _ = _check(got, img, xy, conf, cls, 3, **kw)
    assert keep.sum() >= 2 and (len(img) < 100 or keep.sum() < len(img))


@pytest.mark.parametrize('seed', range(5))
@pytest.mark.parametrize('class_aware', [False, True])
def test_float_corner_lists(seed, class_aware):
    img, xy, conf, cls = R.float_lists(seed)
    kw = dict(iou_th=0.45, class_aware=class_aware)
    keep, _, visited, _ = R.nms(img, xy, conf, cls, n_images=3, **kw)
    assert np.abs(visited - 0.45).min() >= 1e-9, 'precondition: a decision sits on the threshold'
    # roughly a quarter is suppressed; per class (three classes) fewer boxes meet a kept box of their own class
    assert (0.05 if class_aware else 0.15) * len(img) <= (keep == 0).sum() <= 0.4 * len(img)
    _check(_run(img, xy, conf, cls, 3, **kw), img, xy, conf, cls, 3, **kw)


def test_limits_and_repeatability():
    img, xy, conf, cls = R.float_lists(1)
    n = len(img)
    kw = dict(iou_th=0.45, per_image=50)
    # more survivors than slots: the first K are written
    got = _run(img, xy, conf, cls, 3, K=17, **kw)
    keep, _ = _check(got, img, xy, conf, cls, 3, K=17, **kw)
    assert got['count'] == 150 > 17 and keep.sum() == 150
    # fewer survivors than slots: the slots behind them are zero-filled
    got = _run(img, xy, conf, cls, 3, K=n + 9, **kw)
    _check(got, img, xy, conf, cls, 3, K=n + 9, **kw)
    assert not got['xy'][150:].any() and not got['conf'][150:].any() and not got['src'][150:].any()
    # a count beyond the capacity is clamped, a count below the list length cuts the list, entries past it get keep = 0
    got = _run(img, xy, conf, cls, 3, count=n + 1000, **kw)
    _check(got, img, xy, conf, cls, 3, **kw)
    got = _run(img, xy, conf, cls, 3, count=300, **kw)
    _check(dict(got, keep=got['keep'][:300]), img[:300], xy[:300], conf[:300], cls[:300], 3, K=n, **kw)
    assert not got['keep'][300:].any()
    got = _run(img[:300], xy[:300], conf[:300], cls[:300], 3, n_cap=n, K=n, count=300, **kw)     # junk behind the live length
    _check(dict(got, keep=got['keep'][:300]), img[:300], xy[:300], conf[:300], cls[:300], 3, K=n, **kw)
    assert not got['keep'][300:].any()
    got = _run(img, xy, conf, cls, 3, count=-4, **kw)
    assert got['count'] == 0 and not got['keep'].any() and not got['xy'].any() and got['err'] == 0
    # an image over max_per_image: the 2^20 bit, its boxes dropped, the others untouched
    sizes = np.bincount(img, minlength=3)
    cap = int(np.sort(sizes)[1])                                        # the largest image does not fit
    assert sizes.max() > cap
    got = _run(img, xy, conf, cls, 3, max_per_image=cap, **kw)
    keep, _ = _check(got, img, xy, conf, cls, 3, max_per_image=cap, **kw)
    assert got['err'] == 1 << 20 and not keep[img == np.argmax(sizes)].any() and keep.sum() == 100
    # a second call gives identical bytes
    a, b = _run(img, xy, conf, cls, 3, **kw), _run(img, xy, conf, cls, 3, **kw)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k]


def test_nms_boxes_device_wrapper():
    img, xy, conf, cls = R.float_lists(2)
    keep, order, _, _ = R.nms(img, xy, conf, cls, n_images=3, iou_th=0.3, class_aware=True)
    n_kept, o_img, o_xy, o_conf, o_cls, o_src, d_keep = utils.nms_boxes_device(img, xy, conf, cls, iou_th=0.3, class_aware=True)
    assert n_kept == len(order) and int(o_src.numel()) == n_kept
    np.testing.assert_array_equal(d_keep.cpu().numpy(), keep)
    np.testing.assert_array_equal(o_src.cpu().numpy(), order)
    np.testing.assert_array_equal(o_img.cpu().numpy(), img[order])
    np.testing.assert_array_equal(o_xy.cpu().numpy(), xy[order])
    np.testing.assert_array_equal(o_conf.cpu().numpy(), conf[order])
    np.testing.assert_array_equal(o_cls.cpu().numpy(), cls[order])
    few = utils.nms_boxes_device(img, xy, conf, iou_th=0.3, max_out=5, n_images=3)
    assert few[0] == int(R.nms(img, xy, conf, None, n_images=3, iou_th=0.3)[0].sum()) > 5 and int(few[5].numel()) == 5 and few[4] is None
    none = utils.nms_boxes_device(np.zeros(0, np.int32), np.zeros((0, 4)), np.zeros(0, np.float32))
    assert none[0] == 0 and int(none[6].numel()) == 0


# ------------------------------------------------------------------------------------------------ the masked y_hat
def test_nms_y_hat_device():
    y, kw = R.y_hat_case()
    p = make_params(device='cuda', **kw)
    hw = np.array([(80, 100), (64, 72)])
    nb, C = kw['n_boxes'], kw['n_classes']
    n, idx, xy, cls, conf = utils.decode_boxes_device(y, p, hw, 0.0, with_conf=True)
    idx, xy, cls, conf = idx.cpu().numpy(), xy.cpu().numpy(), cls.cpu().numpy(), conf.cpu().numpy()
    where = np.argwhere(y[..., 0:5 * nb:5] > 0)
    assert n == len(where) == 2 * 4 * 4 * 2 - 3                        # all but the negative, the NaN and the zero confidence
    for class_aware in (False, True):
        keep, _, _, _ = R.nms(idx, xy, conf, cls, n_images=2, iou_th=0.45, class_aware=class_aware)
        assert 0 < (keep == 0).sum() < n
        want = y.copy()
        dead = where[keep == 0]
        want[dead[:, 0], dead[:, 1], dead[:, 2], 5 * dead[:, 3]] = 0.0
        got = utils.nms_y_hat_device(torch.from_numpy(y).cuda(), p, 0.45, class_aware, 0, hw)
        assert got.dtype == torch.float32 and got.is_cuda
        assert _same_bits(got.cpu().numpy(), want)                      # the mask is the restatement's, everything else keeps its bits
        # prefix consistency: decoding the masked y_hat at 0.5 gives what suppression of the decode at 0.5 keeps
        m_n, m_idx, m_xy, m_cls, m_conf = utils.decode_boxes_device(got, p, hw, 0.5, with_conf=True)
        h_n, h_idx, h_xy, h_cls, h_conf = utils.decode_boxes_device(y, p, hw, 0.5, with_conf=True)
        k5 = utils.nms_boxes_device(h_idx, h_xy, h_conf, h_cls, iou_th=0.45, class_aware=class_aware, n_images=2)[6].cpu().numpy() == 1
        assert m_n == int(k5.sum()) and 0 < m_n < h_n
        np.testing.assert_array_equal(m_xy.cpu().numpy(), h_xy.cpu().numpy()[k5])
        np.testing.assert_array_equal(m_conf.cpu().numpy(), h_conf.cpu().numpy()[k5])
        np.testing.assert_array_equal(m_idx.cpu().numpy(), h_idx.cpu().numpy()[k5])
    capped = utils.nms_y_hat_device(y, p, 0.45, False, 3, hw)           # at most three boxes of an image stay
    assert ((capped[..., 0:5 * nb:5] > 0).sum(dim=(1, 2, 3)).cpu().numpy() == 3).all()


# ------------------------------------------------------------------------------------------------ the streaming detector
K_PIPE = 8


def _frames(seed, h=80, w=100, n=2):
    return [im[:h, :w] for im in synth.raw_images(n, seed=seed, min_side=max(h, w), max_side=160)]


class _Chain(object):
    """The tiny models of tests/test_gpu_serve.py, and the record rebuilt from the existing pieces plus the two restatements."""

    def __init__(self):
        self.dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
        self.cp = make_params(model='capsule', n_classes=3, device='cuda')
        torch.manual_seed(3)
        self.dark, self.caps = models.DarkNet(self.dp).cuda().eval(), models.CapsuleNet(self.cp).cuda().eval()
        self.conf_th = 0.0                                              # all 16 boxes of a frame pair are candidates
        # an IoU threshold at which something is suppressed: half the largest IoU of an image's most confident box with another
        idx, xy, conf = self.candidates(_frames(41))
        best = 0.0
        for b in range(2):
            mine = np.flatnonzero(idx == b)
            top = mine[np.argmax(conf[mine])]
            best = max([best] + [float(R.box_iou(xy[top], xy[j])) for j in mine if j != top])
        print('largest IoU with a top box: %.6f' % best)
        assert best > 0.02, 'the detector output has no overlapping boxes'
        self.iou_th = best / 2

    def candidates(self, frames):
        packed = predict_fns.PackedImages(frames)
        with torch.no_grad():
            y = self.dark(packed.resize(64, to_nchw=True)).data
        n, idx, xy, _, conf = utils.decode_boxes_device(y, self.dp, packed.hw, self.conf_th, with_conf=True)
        return idx.cpu().numpy().astype(np.int64), xy.cpu().numpy(), conf.cpu().numpy()

    def record(self, frames, K, nms=True, per_frame=0):
        """(record bytes, keep) of the frames from decode -> restated suppression -> rectangles -> crops -> classifier -> pack."""
        packed = predict_fns.PackedImages(frames)
        idx, xy, conf = self.candidates(frames)
        keep = np.ones(len(idx), np.int32)
        order = np.arange(len(idx))
        if nms:
            keep, order, visited, _ = R.nms(idx, xy, conf, None, n_images=len(frames), iou_th=self.iou_th, per_image=per_frame)
            assert not len(visited) or np.abs(visited - self.iou_th).min() > 1e-9       # (per_frame = 1 compares no pair)
        total = len(order)
        s_idx, s_xy, s_conf = np.zeros(K, np.int64), np.zeros((K, 4)), np.zeros(K, np.float32)
        m = min(total, K)
        s_idx[:m], s_xy[:m], s_conf[:m] = idx[order[:m]], xy[order[:m]], conf[order[:m]]
        rect, bad, live = serve_ref.slot_rectangles(total, s_idx, s_xy, packed.hw, K)
        crops = torch.zeros((K, 3, 32, 32), dtype=torch.float32, device='cuda')
        good = np.flatnonzero(live & ~bad)
        if len(good):
            crops[torch.from_numpy(good).cuda()] = packed.crop_resize(s_idx[good], rect[good], 32, 32, -128.0, 1.0 / 128.0, True)
        with torch.no_grad():
            scores = self.caps(crops).data.reshape(K, -1).cpu().numpy()
        return serve_ref.pack(scores, total, s_idx, s_xy, s_conf, rect, int(bad.sum()), 0, K), keep


@pytest.fixture(scope='module')
def chain():
    return _Chain()


def test_sign_detector_with_nms_equals_the_rebuilt_chain(chain):
    frames = _frames(41)
    want, keep = chain.record(frames, K_PIPE)
    assert (keep == 0).sum() >= 1 and keep.sum() >= 2, 'precondition: %d suppressed, %d kept' % ((keep == 0).sum(), keep.sum())
    det = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=K_PIPE, conf_th=chain.conf_th, nms_iou=chain.iou_th)
    res = det.detect(frames)
    np.testing.assert_array_equal(res.record, want)
    assert res.total == int(keep.sum()) and res.n == min(res.total, K_PIPE)
    assert np.all(np.diff(res.image_indices) >= 0)
    for b in (0, 1):
        assert np.all(np.diff(res.conf[res.image_indices == b]) <= 0)
    np.testing.assert_array_equal(det.detect(frames).record, want)       # the same state again
    # two slots and at most one box per frame: the most confident box of each frame
    two = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=2, conf_th=chain.conf_th, nms_iou=chain.iou_th,
                             per_frame=1).detect(frames)
    np.testing.assert_array_equal(two.record, chain.record(frames, 2, per_frame=1)[0])
    idx, xy, conf = chain.candidates(frames)
    assert two.total == 2 and two.conf.tolist() == [conf[idx == 0].max(), conf[idx == 1].max()]


def test_sign_detector_graph_replays_the_suppression_step(chain):
    kw = dict(max_boxes=K_PIPE, conf_th=chain.conf_th, nms_iou=chain.iou_th)
    eager = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, **kw)
    graphed = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, graph=True, **kw)
    records = []
    for seed in (41, 42, 41):
        frames = _frames(seed)
        a, b = eager.detect(frames), graphed.detect(frames)
        np.testing.assert_array_equal(b.record, a.record)
        records.append(a.record)
    assert not np.array_equal(records[0], records[1]) and np.array_equal(records[0], records[2])
    assert len(graphed.states) == 1 and graphed.states[(2, 80, 100)].graph is not None


def test_sign_detector_without_the_arguments_is_unchanged(chain):
    frames = _frames(41)
    for K in (K_PIPE, 20):
        want, _ = chain.record(frames, K, nms=False)                     # the first K boxes in decode order, total = all of them
        res = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, max_boxes=K, conf_th=chain.conf_th).detect(frames)
        np.testing.assert_array_equal(res.record, want)
        assert res.total == 16


# ------------------------------------------------------------------------------------------------ dark_pred / dark_class_pred
def _checkpoints(tmp_path, n_classes_dark=0):
    dp = make_params(model='darknet_d', n_classes=n_classes_dark, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    cp = make_params(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(3)
    dark, caps = models.DarkNet(dp).cuda(), models.CapsuleNet(cp).cuda()
    ddir, cdir = str(tmp_path / 'darknet_d'), str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': dark.state_dict()}, False, ddir)
    utils.save_checkpoint({'epoch': 0, 'state_dict': caps.state_dict()}, False, cdir)
    json.dump(dict(batch_size=4, n_classes=n_classes_dark, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, dropout=0.0),
              open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    return dp, cp, dark, caps, ddir, cdir


def test_dark_pred_and_dark_class_pred_with_nms(tmp_path):
    dp, cp, dark, caps, ddir, cdir = _checkpoints(tmp_path)
    images = synth.raw_images(5)
    hw = np.array([im.shape[0:2] for im in images])
    plain, _ = predict_fns.dark_pred(images, dark, ddir, dp, 'last', batch_size=2)
    conf_th = float(np.median(plain[..., 0::5]))
    iou_th = 0.2
    masked = utils.nms_y_hat_device(plain, dp, iou_th, False, 0, hw)
    y_hat, crops, idx, xy = predict_fns.dark_pred(images, dark, ddir, dp, 'last', is_end=False, conf_th=conf_th, batch_size=2,
                                                  nms_iou=iou_th)
    assert _same_bits(y_hat, masked.cpu().numpy())
    suppressed = int(((plain[..., 0::5] > conf_th) & (y_hat[..., 0::5] == 0)).sum())
    print('%d boxes over %.4f, %d suppressed' % ((plain[..., 0::5] > conf_th).sum(), conf_th, suppressed))
    assert suppressed >= 1, 'precondition: nothing over the threshold is suppressed at IoU %.2f' % iou_th
    # boxes and crops are those of the survivors: the decode of the masked y_hat, which is the suppressed decode of the plain one
    n, m_idx, m_xy, _ = utils.decode_boxes_device(masked, dp, hw, conf_th)
    np.testing.assert_array_equal(idx, m_idx.cpu().numpy())
    np.testing.assert_array_equal(xy, m_xy.cpu().numpy())
    h_n, h_idx, h_xy, _, h_conf = utils.decode_boxes_device(plain, dp, hw, conf_th, with_conf=True)
    k = utils.nms_boxes_device(h_idx, h_xy, h_conf, iou_th=iou_th, n_images=len(images))[6].cpu().numpy() == 1
    assert n == int(k.sum()) == h_n - suppressed
    np.testing.assert_array_equal(xy, h_xy.cpu().numpy()[k])
    packed = predict_fns.PackedImages(images)
    want = packed.crop_resize(idx, utils.crop_rectangles(xy, idx, hw), 32, 32, 0.0, 1.0, False)
    np.testing.assert_array_equal(crops, want.cpu().numpy())
    # the combined chain: its detector part is the masked y_hat, its class part the classifier's scores of the survivors' crops
    both, _ = predict_fns.dark_class_pred(images, dark, ddir, dp, caps, cdir, cp, 'last', batch_size=2, conf_th=conf_th, nms_iou=iou_th)
    D = plain.shape[3]
    assert both.shape[3] == D + 43 and _same_bits(both[..., :D].astype(np.float32), y_hat)
    centred = packed.crop_resize(idx, utils.crop_rectangles(xy, idx, hw), 32, 32, -128.0, 1.0 / 128.0, True)
    with torch.no_grad():
        scores = torch.cat([caps.eval()(centred[lo:lo + 2]).data.reshape(-1, 43) for lo in range(0, n, 2)])
    want = utils.combine_y_hat_device(hw, masked, scores, idx, xy, dp)
    np.testing.assert_array_equal(both, want.cpu().numpy().astype(np.float64))
    # without the argument nothing changes
    again, _ = predict_fns.dark_pred(images, dark, ddir, dp, 'last', batch_size=2)
    assert _same_bits(again, plain)


# ------------------------------------------------------------------------------------------------ the command line
def test_main_serve_and_detect_with_nms(tmp_path, capsys):
    _, _, _, _, ddir, _ = _checkpoints(tmp_path)
    spec = importlib.util.spec_from_file_location('cy_main_nms', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    common = ['--model', 'darknet_d', '--synthetic', '3', '--model_dir', ddir, '--restore', 'last']
    plain = m.main(['--mode', 'serve', '--combine', 'capsule'] + common)
    out = m.main(['--mode', 'serve', '--combine', 'capsule', '--nms', '0.45', '--per_frame', '2', '--graph'] + common)
    lines = open(os.path.join(ddir, 'serve_output.txt')).read().splitlines()
    assert len(lines) == 3 and [ln.split(':')[0] for ln in lines] == ['frame 0', 'frame 1', 'frame 2']
    found = [int(ln.split(' of ')[1].split(' |')[0]) for ln in lines]
    assert out['frames'] == 3 and out['boxes'] <= plain['boxes'] and all(f <= 2 for f in found)
    capsys.readouterr()
    res = m.main(['--mode', 'detect', '--nms', '0.45'] + common)
    text = open(os.path.join(ddir, 'metric_output.txt')).read()
    fields = dict(f.split(':') for f in text.split(', ') if f)
    assert list(fields) == ['detect_AP', 'detect_acc'] == list(res)
    assert all(np.isfinite(float(v)) and 0.0 <= float(v) <= 1.0 for v in fields.values())
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('nms (iou > 0.45)')]
    assert len(said) == 1 and 'boxes over 0.5 suppressed' in said[0]
    with pytest.raises(SystemExit, match='--nms_class_aware'):          # this detector has no class scores
        m.main(['--mode', 'detect', '--nms', '0.45', '--nms_class_aware'] + common)

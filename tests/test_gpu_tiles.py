"""GPU tests of tiled detection: `cy_yolo_decode_tiles_conf` (csrc/tiles.hip) against the numpy restatement tests/tiles_ref.py and
against the existing decode kernel, serve.SignDetector(tiles=) against the untiled detector and against the chain of existing pieces,
predict_fns.dark_pred_tiled with metrics.detect_report_boxes, and augment.AugmentFeeder(tiles=)."""
import numpy as np
import pytest
import torch

from helpers import make_params

import tiles_ref as R
from augment_ref import center, paste_resize_ref
from capsyolo_amd import augment, metrics, models, predict_fns, serve, synth, utils
from capsyolo_amd.predict_fns import PackedImages
from capsyolo_amd.tiles import TileSpec, tile_rects
from test_gpu_serve import K_PIPE, _Chain, _frames

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the kernel
CONF_TH = 0.5
MARGINS = (-1.0, 0.0, 2.0)


def _tables(frame_hw, rows, cols, overlap, full):
    tables = [tile_rects(h, w, rows, cols, overlap, full) for h, w in frame_hw]
    return np.concatenate([np.full(len(t), k, np.int32) for k, t in enumerate(tables)]), np.concatenate(tables)


def _random_y(Bt, g, nb, C, seed):
    """Uniform [0, 1) float32 with the width and height columns scaled by 0.3: about half the boxes pass 0.5, and a box is at most
    0.3 of its tile wide, so the boxes of the border cells reach over a tile's edge or stay clear of it about equally often."""
    y = np.random.default_rng(seed).random((Bt, g, g, 5 * nb + C), dtype=np.float32)
    for k in range(nb):
        y[..., 5 * k + 3:5 * k + 5] *= np.float32(0.3)
    return y


# name -> (y, n_classes, tile_frame, tile_rect, frame_hw)
def _kernel_cases():
    two = [(80, 100), (90, 120)]
    cases = {}
    tf, tr = _tables(two, 2, 2, 16, True)                                 # 2 frames x (2 x 2 + full) = 10 tiles, 180 cells: one pass
    cases['one_pass'] = (_random_y(10, 3, 2, 0, 1), 0, tf, tr, two)
    tf, tr = _tables(two, 2, 3, 12, False)                                # 12 tiles, 1176 cells: the 1024 boundary is crossed
    cases['two_passes'] = (_random_y(12, 7, 2, 3, 2), 3, tf, tr, two)
    y = np.zeros((1, 1, 1, 5), np.float32)                                # one cell: its box reaches over the left edge of an inner tile
    y[0, 0, 0] = [0.9, 0.25, 0.5, 0.75, 0.25]
    cases['one_cell'] = (y, 0, np.array([0], np.int32), np.array([[16, 64, 20, 70]], np.int32), [(80, 100)])
    return cases


KERNEL_CASES = _kernel_cases()
_REF = {}


def _ref(name, margin):
    """The restatement's answer, computed once per (case, margin) and shared."""
    if (name, margin) not in _REF:
        y, C, tf, tr, hw = KERNEL_CASES[name]
        _REF[(name, margin)] = R.decode_tiles(y, C, tf, tr, hw, CONF_TH, margin)
    return _REF[(name, margin)]


def _run(name, margin, max_boxes=None):
    y, C, tf, tr, hw = KERNEL_CASES[name]
    p = make_params(n_classes=C, darknet_input=64, device='cuda')
    out = utils.decode_tiles_device(y, p, tf, tr, hw, CONF_TH, margin, with_tile=True, max_boxes=max_boxes)
    n, idx, xy, cls, conf, dropped, tile = out
    return n, dropped, [None if t is None else t.cpu().numpy() for t in (idx, xy, cls, conf, tile)]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_preconditions_of_the_kernel_cases():
    """Checked with the restatement alone: every multi-cell case with margin >= 0 keeps some boxes and drops some (the one-cell case
    holds ONE box, which margin 2 drops and margin -1 keeps), each of the four sides fires, the second case has hits on both sides
    of the 1024-cell boundary."""
    fired = dict.fromkeys(R.SIDES, 0)
    for name in ('one_pass', 'two_passes'):
        for margin in (0.0, 2.0):
            ref = _ref(name, margin)
            print(name, margin, ref['count'], ref['dropped'], ref['fired'])
            assert ref['count'] > 0 and ref['dropped'] > 0 and ref['err'] == 0
            for s in R.SIDES:
                fired[s] += ref['fired'][s]
        off = _ref(name, -1.0)
        assert off['dropped'] == 0 and off['count'] == _ref(name, 2.0)['count'] + _ref(name, 2.0)['dropped']
    assert all(fired[s] > 0 for s in R.SIDES), fired
    assert (_ref('one_cell', 2.0)['count'], _ref('one_cell', 2.0)['dropped']) == (0, 1) and _ref('one_cell', 2.0)['fired']['left'] == 1
    assert (_ref('one_cell', 0.0)['count'], _ref('one_cell', 0.0)['dropped']) == (0, 1)
    assert (_ref('one_cell', -1.0)['count'], _ref('one_cell', -1.0)['dropped']) == (1, 0)
    y = KERNEL_CASES['two_passes'][0]
    cells = (y[..., 0:10:5] > np.float32(CONF_TH)).reshape(-1)            # (tile, row, column, box) order
    assert cells.size == 1176 and cells[:1024].any() and cells[1024:].any()
    tiles_of_kept = _ref('two_passes', 2.0)['tile']
    assert (tiles_of_kept * 98 < 1024).any() and (tiles_of_kept * 98 >= 1024).any()


@pytest.mark.parametrize('margin', MARGINS)
@pytest.mark.parametrize('name', sorted(KERNEL_CASES))
def test_decode_tiles_against_the_restatement_and_the_existing_decode(name, margin):
    y, C, tf, tr, hw = KERNEL_CASES[name]
    ref = _ref(name, margin)
    n, dropped, (idx, xy, cls, conf, tile) = _run(name, margin)
    # yardstick 1: the restatement -- everything but xy exactly, xy within the tolerance of the existing decode test
    assert (n, dropped) == (ref['count'], ref['dropped'])
    assert _same_bits(idx, ref['idx']) and _same_bits(conf, ref['conf']) and _same_bits(tile, ref['tile'])
    assert (cls is None and ref['cls'] is None) if C == 0 else _same_bits(cls, ref['cls'])
    np.testing.assert_allclose(xy, ref['xy'], rtol=1e-14, atol=1e-11)
    assert np.all(np.diff(idx) >= 0)                                      # frame ascending: what cy_nms_boxes needs
    # yardstick 2: the existing decode kernel with the tile sizes as the image sizes, the rule and the offset in numpy: bit for bit
    p = make_params(n_classes=C, darknet_input=64, device='cuda')
    sizes = np.stack([tr[:, 1] - tr[:, 0], tr[:, 3] - tr[:, 2]], axis=1)
    e_n, e_idx, e_xy, e_cls, e_conf = utils.decode_boxes_device(y, p, sizes, CONF_TH, with_conf=True)
    e_idx, e_xy, e_conf = e_idx.cpu().numpy(), e_xy.cpu().numpy(), e_conf.cpu().numpy()
    assert e_n == n + dropped
    hw_a = np.asarray(hw)
    keep = np.array([not any(R.border_sides(e_xy[i], tr[b], hw_a[tf[b], 0], hw_a[tf[b], 1], margin)) for i, b in enumerate(e_idx)], dtype=bool)
    off = np.stack([tr[e_idx, 2], tr[e_idx, 0], tr[e_idx, 2], tr[e_idx, 0]], axis=1).astype(np.float64)
    assert _same_bits(xy, np.ascontiguousarray((e_xy + off)[keep].reshape(-1, 4)))
    assert _same_bits(tile, e_idx[keep].astype(np.int32)) and _same_bits(conf, e_conf[keep])
    if C:
        assert _same_bits(cls, e_cls.cpu().numpy()[keep])
    # a second run gives identical bytes
    n2, dropped2, again = _run(name, margin)
    assert (n2, dropped2) == (n, dropped)
    for a, b in zip((idx, xy, cls, conf, tile), again):
        assert (a is None and b is None) or _same_bits(a, b)


@pytest.mark.parametrize('margin', MARGINS)
def test_decode_tiles_with_fewer_slots_than_boxes(margin):
    ref = _ref('two_passes', margin)
    slots = ref['count'] // 2
    assert slots >= 1
    n, dropped, (idx, xy, cls, conf, tile) = _run('two_passes', margin, max_boxes=slots)
    assert (n, dropped) == (ref['count'], ref['dropped']) and len(idx) == slots          # the count says how many there were
    assert _same_bits(idx, ref['idx'][:slots]) and _same_bits(conf, ref['conf'][:slots]) and _same_bits(tile, ref['tile'][:slots])
    assert _same_bits(cls, ref['cls'][:slots])
    np.testing.assert_allclose(xy, ref['xy'][:slots], rtol=1e-14, atol=1e-11)
    full = _run('two_passes', margin)[2]
    assert _same_bits(xy, full[1][:slots])


def test_decode_tiles_counts_bad_tiles():
    y, C, tf, tr, hw = KERNEL_CASES['one_pass']
    p = make_params(n_classes=C, darknet_input=64, device='cuda')
    bad_tf, bad_tr = tf.copy(), tr.copy()
    bad_tf[9] = 2                                                         # a frame that does not exist (still ascending)
    bad_tr[3] = [32, 81, 42, 100]                                         # leaves its 80 x 100 frame
    bad_tr[6] = [10, 10, 0, 50]                                           # empty
    want = R.decode_tiles(y, C, bad_tf, bad_tr, hw, CONF_TH, 2.0)
    assert want['err'] == 3 and want['count'] > 0
    with pytest.raises(ValueError, match='3 tile'):
        utils.decode_tiles_device(y, p, bad_tf, bad_tr, hw, CONF_TH, 2.0)


# ------------------------------------------------------------------------------------------------ the streaming detector
@pytest.fixture(scope='module')
def chain():
    return _Chain()


def test_one_by_one_tiling_is_the_untiled_detector(chain):
    kw = dict(max_boxes=K_PIPE, conf_th=chain.conf_th, nms_iou=0.45)
    plain = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, **kw).detect(chain.frames)
    tiled = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, tiles=TileSpec(1, 1, 0), **kw).detect(chain.frames)
    assert plain.n >= 1
    np.testing.assert_array_equal(tiled.record, plain.record)


SPEC = TileSpec(2, 2, 16, full=True)


class _TiledChain(object):
    """The tiled pipeline from the existing pieces, for the frames and models of `chain`: the candidates of every window at
    confidence > 0, and for a threshold the survivors with their crops."""

    def __init__(self, chain, frames):
        self.chain, self.frames = chain, frames
        self.packed = PackedImages(frames)
        self.tf, self.tr = _tables(self.packed.hw, SPEC.rows, SPEC.cols, SPEC.overlap, SPEC.full)
        assert len(self.tf) == 10
        with torch.no_grad():
            x = self.packed.crop_resize(self.tf, self.tr, 64, 64, 0.0, 1.0, True)
            self.y = chain.dark(x).data
        sizes = np.stack([self.tr[:, 1] - self.tr[:, 0], self.tr[:, 3] - self.tr[:, 2]], axis=1)
        n, t_idx, t_xy, _, t_conf = utils.decode_boxes_device(self.y, chain.dp, sizes, 0.0, with_conf=True)
        assert n == 80                                                    # every box of every window has a confidence > 0
        t_idx, t_xy, self.t_conf = t_idx.cpu().numpy(), t_xy.cpu().numpy(), t_conf.cpu().numpy()
        hw = self.packed.hw
        self.cut = np.array([any(R.border_sides(t_xy[i], self.tr[b], hw[self.tf[b], 0], hw[self.tf[b], 1], SPEC.margin))
                             for i, b in enumerate(t_idx)], dtype=bool)
        off = np.stack([self.tr[t_idx, 2], self.tr[t_idx, 0], self.tr[t_idx, 2], self.tr[t_idx, 0]], axis=1).astype(np.float64)
        self.f_idx, self.f_xy = self.tf[t_idx], t_xy + off

    def at(self, conf_th, K):
        """(candidates over conf_th, dropped by the border rule, survivors, idx, xy, conf, crops) at a threshold."""
        over = self.t_conf > np.float32(conf_th)
        live = over & ~self.cut
        if not live.any():
            return int(over.sum()), int((over & self.cut).sum()), 0, None, None, None, None
        kept, idx, xy, conf, _, _, _ = utils.nms_boxes_device(self.f_idx[live], self.f_xy[live], self.t_conf[live], None, iou_th=0.45,
                                                              n_images=self.packed.n, max_out=K)
        idx, xy, conf = idx.cpu().numpy().astype(np.int64), xy.cpu().numpy(), conf.cpu().numpy()
        rect = utils.crop_rectangles(xy, idx, self.packed.hw)
        crops = self.packed.crop_resize(idx, rect, 32, 32, -128.0, 1.0 / 128.0, True)
        return int(over.sum()), int((over & self.cut).sum()), kept, idx, xy, conf, crops

    def threshold(self, K):
        """Between two neighbouring distinct confidences, as the untiled pipeline test chooses it: the highest such threshold at which
        between 1 and K - 1 boxes survive and at least one candidate is suppressed or dropped."""
        conf = np.unique(self.t_conf)[::-1].astype(np.float64)
        for j in range(1, len(conf)):
            th = float(conf[j - 1] + conf[j]) / 2
            over, dropped, kept = self.at(th, K)[:3]
            print('threshold %.6f: %d candidates, %d dropped, %d survive' % (th, over, dropped, kept))
            if kept > K - 1:
                break
            if kept >= 1 and over - kept >= 1:
                return th
        raise AssertionError('precondition: no threshold with 1..%d survivors and a suppressed or dropped candidate' % (K - 1))


@pytest.fixture(scope='module')
def tiled(chain):
    return _TiledChain(chain, chain.frames)


def test_tiled_pipeline_equals_the_chain_of_existing_pieces(chain, tiled):
    K = K_PIPE
    th = tiled.threshold(K)
    over, dropped, n, idx, xy, conf, crops = tiled.at(th, K)
    assert 1 <= n <= K - 1 and over - n >= 1
    kw = dict(max_boxes=K, conf_th=th, nms_iou=0.45, tiles=SPEC)
    det = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, **kw)
    res = det.detect(chain.frames)
    assert (res.n, res.total, res.truncated, res.bad) == (n, n, False, {'boxes': 0, 'frames': 0})
    np.testing.assert_array_equal(res.image_indices, idx)
    np.testing.assert_array_equal(res.boxes_xy, xy)
    np.testing.assert_array_equal(res.conf, conf)
    words = det.states[(2, 80, 100)].cand.words.cpu().numpy()
    assert words[0] == over - dropped and words[1] == 0 and words[4] == dropped and words[5] == 0
    with torch.no_grad():
        padded = torch.cat([crops, torch.zeros((K - n, 3, 32, 32), dtype=torch.float32, device='cuda')])
        scores = chain.caps(padded).data.reshape(K, -1).cpu().numpy()[:n]
        alone = chain.caps(crops).data.reshape(n, -1).cpu().numpy()
    np.testing.assert_array_equal(res.classes, np.argmax(scores, axis=1))
    np.testing.assert_array_equal(res.class_scores, scores[np.arange(n), np.argmax(scores, axis=1)])
    top = np.sort(alone.astype(np.float64), axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-3
    assert clear.any() and np.array_equal(res.classes[clear], np.argmax(alone, axis=1)[clear])
    np.testing.assert_array_equal(det.detect(chain.frames).record, res.record)           # a second call
    graphed = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, graph=True, **kw)
    np.testing.assert_array_equal(graphed.detect(chain.frames).record, res.record)       # the capturing call
    np.testing.assert_array_equal(graphed.detect(chain.frames).record, res.record)       # a replay
    other = _frames(42)
    np.testing.assert_array_equal(graphed.detect(other).record, det.detect(other).record)
    assert len(graphed.states) == 1 and graphed.states[(2, 80, 100)].graph is not None


def test_tiled_detector_with_per_frame_and_class_aware(chain):
    """per_frame caps a frame's survivors; nms_class_aware suppresses inside the detector's own arg-max class."""
    kw = dict(max_boxes=K_PIPE, conf_th=0.0, nms_iou=0.45, tiles=SPEC)
    free = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, **kw).detect(chain.frames)
    capped = serve.SignDetector(chain.dark, chain.dp, chain.caps, chain.cp, per_frame=1, **kw).detect(chain.frames)
    assert capped.n == capped.total == 2 and capped.image_indices.tolist() == [0, 1] and free.total > 2
    np.testing.assert_array_equal(capped.boxes_xy[0], free.boxes_xy[0])   # a frame's most confident survivor
    rp = make_params(model='darknet_r', n_classes=3, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    torch.manual_seed(4)
    dark_r = models.DarkNet(rp).cuda().eval()
    res = serve.SignDetector(dark_r, rp, chain.caps, chain.cp, nms_class_aware=True, **kw).detect(chain.frames)
    packed = PackedImages(chain.frames)
    tf, tr = _tables(packed.hw, SPEC.rows, SPEC.cols, SPEC.overlap, SPEC.full)
    with torch.no_grad():
        y = dark_r(packed.crop_resize(tf, tr, 64, 64, 0.0, 1.0, True)).data
    n, idx, xy, cls, conf, dropped = utils.decode_tiles_device(y, rp, tf, tr, packed.hw, 0.0, SPEC.margin)
    kept, w_idx, w_xy, w_conf, _, _, _ = utils.nms_boxes_device(idx, xy, conf, cls, iou_th=0.45, class_aware=True, n_images=2, max_out=K_PIPE)
    assert n + dropped == 80 and res.total == kept >= 1
    np.testing.assert_array_equal(res.image_indices, w_idx.cpu().numpy())
    np.testing.assert_array_equal(res.boxes_xy, w_xy.cpu().numpy())
    np.testing.assert_array_equal(res.conf, w_conf.cpu().numpy())


# ------------------------------------------------------------------------------------------------ evaluation
def test_dark_pred_tiled_and_detect_report_boxes(chain, tiled, tmp_path):
    ddir = str(tmp_path / 'darknet_d')
    utils.save_checkpoint({'epoch': 0, 'state_dict': chain.dark.state_dict()}, False, ddir)
    frames = _frames(41) + _frames(44, 64, 72, 1)                         # three frames of two sizes
    hw = np.array([f.shape[0:2] for f in frames])
    # labels that the detector's boxes hit at the IoU thresholds up to 0.7 and miss above (a random detector hits no random label):
    # the untiled survivors at confidence > 0, every box concentric with 0.85 of its width and height (IoU 0.7225), confidence 1
    y_hat, _ = predict_fns.dark_pred(frames, chain.dark, ddir, chain.dp, 'last', batch_size=2, nms_iou=0.45)
    y = y_hat.astype(np.float64)
    for k in (0, 5):
        y[..., k] = y[..., k] > 0
        y[..., k + 3:k + 5] *= 0.85
    _, g_idx, g_xy, _, g_conf = utils.decode_boxes_device(y, chain.dp, hw, 0.0, with_conf=True)
    gt = (g_idx.cpu().numpy(), g_xy.cpu().numpy(), g_conf.cpu().numpy())
    assert len(gt[0]) == int((y_hat[..., 0::5] > 0).sum()) >= 3
    merged, drawn = predict_fns.dark_pred_tiled(frames, chain.dark, ddir, chain.dp, 'last', SPEC, 0.45, y=y, batch_size=10, draw=True)
    idx, xy, conf, cls = merged
    assert cls is None and len(idx) >= 3 and set(idx.tolist()) == {0, 1, 2} and np.all(np.diff(idx) >= 0)
    for f in range(3):
        assert np.all(np.diff(conf[idx == f]) <= 0)                       # inside an image confidence descending
    assert len(drawn) == 3 and [d.shape for d in drawn] == [f.shape for f in frames]
    # the chunking (two frames, then one) does not show: the first two frames are what the pipeline's chain of pieces gives
    live = ~tiled.cut
    _, w_idx, w_xy, w_conf, _, _, _ = utils.nms_boxes_device(tiled.f_idx[live], tiled.f_xy[live], tiled.t_conf[live], None, iou_th=0.45,
                                                             n_images=2)
    two = idx < 2
    np.testing.assert_array_equal(xy[two], w_xy.cpu().numpy())
    np.testing.assert_array_equal(conf[two], w_conf.cpu().numpy())
    # the sweep over the merged list against the numpy sweep: integer counts equal.  Ground truth: the labels above, and every
    # second box of the merged list itself shrunk the same way, so that the tiled boxes hit some of it
    cx, cy, w, h = (xy[::2, 0] + xy[::2, 2]) / 2, (xy[::2, 1] + xy[::2, 3]) / 2, 0.85 * (xy[::2, 2] - xy[::2, 0]), 0.85 * (xy[::2, 3] - xy[::2, 1])
    near = (idx[::2], np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1), np.ones(len(cx), np.float32))
    conf_ths, iou_ths = np.concatenate([np.linspace(0, 1, 100), [0.5]]), np.linspace(0.5, 0.95, 10)
    for truth in (gt, near):
        got = metrics.confusion_sweep_boxes(truth, merged[:3], 3, conf_ths, iou_ths)
        want = R.confusion_sweep(truth, merged[:3], 3, conf_ths, iou_ths)
        assert got.shape == (101, 1, 10, 3) and got.dtype == np.int64
        np.testing.assert_array_equal(got[:, 0], want)
        assert np.all(want[0, :, 0] + want[0, :, 2] == len(truth[0]))     # TP + FN = the ground truth
    print('hits of the shrunk boxes per IoU threshold at confidence > 0: %s' % want[0, :, 0].tolist())
    assert want[0, 0, 0] == len(near[0]) and want[0, 9, 0] == 0 and want[0, 0, 1] > 0 and want[100, 0, 0] <= len(near[0])
    report = metrics.detect_report_boxes(near, merged[:3], 3)
    assert list(report) == ['detect_AP', 'detect_acc'] and 0.0 < report['detect_AP'] < 1.0
    # 1 x 1 tiles and the same suppression: the report of the untiled path
    one, _ = predict_fns.dark_pred_tiled(frames, chain.dark, ddir, chain.dp, 'last', TileSpec(1, 1, 0), 0.45, batch_size=2)
    assert len(one[0]) == len(gt[0])
    want = metrics.detect_report(y, y_hat, chain.dp)
    assert metrics.detect_report_boxes(gt, one[:3], 3) == want and 0.0 < want['detect_AP'] < 1.0


def test_confusion_sweep_is_confusion_sweep_boxes_on_the_decoded_lists():
    p = make_params(n_classes=3, n_grid=2, n_boxes=2, darknet_input=64, device='cuda')
    rng = np.random.default_rng(3)
    y, y_hat = rng.random((4, 2, 2, 13), dtype=np.float32), rng.random((4, 2, 2, 13), dtype=np.float32)
    conf_ths, iou_ths = np.linspace(0, 1, 7), [0.1, 0.3, 0.5]
    lists = []
    for arr in (y, y_hat):
        _, idx, xy, cls, conf = utils.decode_boxes_device(arr, p, None, 0.0, with_conf=True)
        lists.append((idx, xy, conf, cls))
    for per_class in (True, False):
        want = metrics.confusion_sweep(y, y_hat, p, conf_ths, iou_ths, per_class=per_class)
        got = metrics.confusion_sweep_boxes(lists[0], lists[1], 4, conf_ths, iou_ths, 3 if per_class else 0)
        np.testing.assert_array_equal(got, want)
        assert want.shape == (7, 3 if per_class else 1, 3, 3) and want[..., 0].sum() > 0
    np.testing.assert_array_equal(metrics.confusion_sweep_boxes(lists[0][:3], lists[1][:3], 4, conf_ths, iou_ths)[:, 0],
                                  R.confusion_sweep([a.cpu().numpy() for a in lists[0][:3]], [a.cpu().numpy() for a in lists[1][:3]], 4,
                                                    conf_ths, iou_ths))


# ------------------------------------------------------------------------------------------------ training on the windows
def test_augment_feeder_with_tiles():
    frames = synth.raw_images(8)
    boxes = synth.raw_boxes(frames)
    bank = augment.SignBank(*synth.sign_bank(6))
    packed = PackedImages(frames)
    spec = TileSpec(2, 2, 8, full=True)
    batches = [np.array([5, 2, 7, 0]), np.array([1, 3, 6, 4])]
    feeder = augment.AugmentFeeder(packed, boxes, bank, batches, 64, 2, 43, add_signs=2, seed=1, epoch=0, tiles=spec)
    plain = augment.AugmentFeeder(packed, boxes, bank, batches, 64, 2, 43, add_signs=2, seed=1, epoch=0)
    windows = 0
    for (x, y), idx in zip(feeder, batches):
        rect, begin, pastes, y_plan = feeder.plan(idx)
        assert np.array_equal(pastes, plain.plan(idx)[2]) and np.array_equal(begin, plain.plan(idx)[1])     # the same pastes
        assert tuple(x.shape) == (4, 3, 64, 64) and x.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), y_plan)
        assert torch.equal(x, augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, 64, 64, 'f32_nchw'))
        want = paste_resize_ref(frames, bank.images, idx, rect, begin, pastes, 64, 64)                      # the window as the source
        got = augment.paste_resize_device(packed, bank, idx, rect, begin, pastes, 64, 64, 'u8')
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(x.cpu().numpy(), center(want).transpose(0, 3, 1, 2))
        for k, f in enumerate(idx):
            rng = augment.sample_rng(1, f, 0)
            _, bx, cl = augment.plan_pastes(rng, boxes[f][:, 0:4], packed.hw[f], bank, 2)
            table = spec.rects(*packed.hw[f])
            assert rect[k].tolist() == table[int(rng.integers(0, len(table)))].tolist()
            assert np.array_equal(y_plan[k], augment.window_labels(bx, cl, rect[k], 64, 2, 43))
            windows += int(rect[k].tolist() != [0, packed.hw[f][0], 0, packed.hw[f][1]])
    assert windows >= 4                                                   # most samples are windows, not the full view


# ------------------------------------------------------------------------------------------------ the command line
def test_main_serve_detect_and_train_with_tiles(tmp_path):
    import importlib.util
    import json
    import os
    from helpers import REPO
    dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    cp = make_params(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(3)
    ddir, cdir = str(tmp_path / 'darknet_d'), str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.DarkNet(dp).state_dict()}, False, ddir)
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.CapsuleNet(cp).state_dict()}, False, cdir)
    json.dump(dict(batch_size=4, n_epochs=1, lr_decay=0.5, l_coord=5, l_noobj=0.5, n_classes=0, n_grid=2, n_boxes=2, darknet_input=64,
                   capsule_input=32, dropout=0.0, add_signs=1), open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_tiles', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    common = ['--model', 'darknet_d', '--synthetic', '3', '--model_dir', ddir, '--restore', 'last']
    tiles = ['--nms', '0.45', '--tiles', '2x2', '--tile_overlap', '8', '--tile_full']
    out = m.main(['--mode', 'serve', '--combine', 'capsule', '--graph'] + tiles + common)
    lines = open(os.path.join(ddir, 'serve_output.txt')).read().splitlines()
    assert out['frames'] == 3 and [ln.split(':')[0] for ln in lines] == ['frame 0', 'frame 1', 'frame 2']
    res = m.main(['--mode', 'detect'] + tiles + common)
    fields = dict(f.split(':') for f in open(os.path.join(ddir, 'metric_output.txt')).read().split(', ') if f)
    assert list(fields) == ['detect_AP', 'detect_acc'] == list(res)
    assert all(np.isfinite(float(v)) and 0.0 <= float(v) <= 1.0 for v in fields.values())
    assert sorted(os.listdir(os.path.join(ddir, 'output'))) == ['0.ppm', '1.ppm', '2.ppm']
    losses_tr, losses_ev = m.main(['--model', 'darknet_d', '--synthetic', '8', '--n_epochs', '1', '--batch_size', '4', '--no_metric', '--model_dir',
                                   ddir, '--augment', '--tiles', '2x2', '--tile_overlap', '8'])
    assert len(losses_tr) == 1 and np.isfinite(losses_tr[0]) and np.isfinite(losses_ev[0])

"""CPU tests of tiled detection: the tile table (capsyolo_amd/tiles.py), the exports and host-side refusals of
`cy_yolo_decode_tiles_conf` (csrc/tiles.hip), hand-made known answers of the numpy restatement tests/tiles_ref.py, the window labels
and the window draw of the augmentation plan, and the refusals of serve.SignDetector(tiles=) that come before any device work."""
import os
import re
import types

import numpy as np
import pytest

from helpers import REPO

import tiles_ref as R
from capsyolo_amd import _lib, augment, serve, synth
from capsyolo_amd.tiles import TileSpec, parse_tiles, tile_rects

# ------------------------------------------------------------------------------------------------ the tile table


def test_tile_rects_known_answers():
    r = tile_rects(800, 1360, 2, 3, 128)
    assert r.dtype == np.int32 and r.shape == (6, 4)
    assert r.tolist() == [[y, y + 464, x, x + 539] for y in (0, 336) for x in (0, 410, 821)]
    assert tile_rects(800, 1360, 1, 1, 0).tolist() == [[0, 800, 0, 1360]]
    assert tile_rects(80, 100, 1, 1, 0, full=True).tolist() == [[0, 80, 0, 100]] * 2
    full = tile_rects(800, 1360, 2, 3, 128, full=True)
    assert np.array_equal(full[:6], r) and full[6].tolist() == [0, 800, 0, 1360]
    assert tile_rects(80, 100, 2, 2, 16).tolist() == [[0, 48, 0, 58], [0, 48, 42, 100], [32, 80, 0, 58], [32, 80, 42, 100]]


def test_tile_rects_cover_with_equal_sizes_and_the_overlap_asked_for():
    n = 0
    for H in (7, 16, 33, 80):
        for W in (9, 31, 100):
            for rows in (1, 2, 3, 4):
                for cols in (1, 2, 5):
                    for ov in (0, 1, 3, 8):
                        try:
                            r = tile_rects(H, W, rows, cols, ov)
                        except ValueError:
                            continue
                        n += 1
                        assert r.shape == (rows * cols, 4)
                        hs, ws = np.unique(r[:, 1] - r[:, 0]), np.unique(r[:, 3] - r[:, 2])
                        assert len(hs) == 1 and len(ws) == 1                           # all tiles of one size
                        assert r[:, 0].min() == 0 and r[:, 1].max() == H and r[:, 2].min() == 0 and r[:, 3].max() == W
                        covered = np.zeros((H, W), bool)
                        for y0, y1, x0, x1 in r:
                            covered[y0:y1, x0:x1] = True
                        assert covered.all()
                        grid = r.reshape(rows, cols, 4)                                # row-major
                        assert np.all(grid[:-1, :, 1] - grid[1:, :, 0] >= ov) and np.all(grid[:, :-1, 3] - grid[:, 1:, 2] >= ov)
                        assert np.all(np.diff(grid[:, 0, 0]) >= 0) and np.all(np.diff(grid[0, :, 2]) >= 0)
    assert n > 300


@pytest.mark.parametrize('args', [(80, 100, 0, 2, 4), (80, 100, 2, 0, 4), (80, 100, 2, 2, -1), (80, 100, 1, 1, 80), (8, 100, 3, 1, 8),
                                  (0, 100, 1, 1, 0), (80, 100, 1.5, 2, 4), (80, 100, 1, 2, 100)])
def test_tile_rects_refusals(args):
    with pytest.raises(ValueError, match='tile_rects'):
        tile_rects(*args)


def test_tile_spec_and_parse():
    t = TileSpec(2, 3, 128)
    assert (t.rows, t.cols, t.overlap, t.full, t.margin, t.n_tiles) == (2, 3, 128, False, 2.0, 6)
    assert TileSpec(2, 3, 128, full=True).n_tiles == 7 and np.array_equal(t.rects(800, 1360), tile_rects(800, 1360, 2, 3, 128))
    assert parse_tiles('2x3') == (2, 3) and parse_tiles(' 1X1 ') == (1, 1)
    for bad in ('2', 'x3', '0x2', '2x-1', 'axb', '2x3x4'):
        with pytest.raises(ValueError, match='--tiles'):
            parse_tiles(bad)
    for bad in ((0, 1, 0), (1, 1, -1), (1.5, 1, 0)):
        with pytest.raises(ValueError, match='TileSpec'):
            TileSpec(*bad)
    with pytest.raises(ValueError, match='margin'):
        TileSpec(1, 1, 0, margin=float('nan'))
    assert t.check_capacity(13, 2, 3413) == 6 * 169 * 2
    with pytest.raises(ValueError, match='7 tiles x 13 x 13 cells x 3 boxes = 3549 candidates per frame, the suppression step holds 3413'):
        TileSpec(2, 3, 128, full=True).check_capacity(13, 3, 3413)


# ------------------------------------------------------------------------------------------------ the entry point
ARGS = ('y', 'tile_frame', 'tile_rect', 'frame_hw', 'n_frames', 'margin', 'Bt', 'g', 'nb', 'C', 'conf_th', 'count', 'dropped', 'image_idx',
        'xy', 'cls', 'conf', 'out_tile', 'max_boxes', 'err')


def test_entry_point_is_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    assert re.search(r'\bint cy_yolo_decode_tiles_conf\(', header)
    assert 'cy_yolo_decode_tiles_conf' in _lib.EXPORTS and hasattr(lib, 'cy_yolo_decode_tiles_conf')
    assert len(_lib._SIGS['cy_yolo_decode_tiles_conf']) == len(ARGS) + 1
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6
    assert 'tiles.hip' in open(os.path.join(REPO, 'cs231-capsule-yolo-traffic-sign-detection_amd', 'csrc', 'Makefile')).read()


def _args(**kw):
    """A call with plausible non-null pointers (never dereferenced on the host; the refusals come before the launch)."""
    a = dict(y=8, tile_frame=8, tile_rect=8, frame_hw=8, n_frames=2, margin=2.0, Bt=4, g=3, nb=2, C=0, conf_th=0.5, count=8, dropped=8,
             image_idx=8, xy=8, cls=None, conf=8, out_tile=None, max_boxes=16, err=8)
    a.update(kw)
    return [a[k] for k in ARGS] + [None]


@pytest.mark.parametrize('kw,msg', [(dict(y=None), 'null argument (y)'), (dict(tile_frame=None), 'tile_frame'),
                                    (dict(tile_rect=None), 'tile_rect'), (dict(frame_hw=None), 'frame_hw'),
                                    (dict(count=None), 'count'), (dict(dropped=None), 'dropped'), (dict(err=None), 'err'),
                                    (dict(image_idx=None), 'image_idx'), (dict(xy=None), 'xy'), (dict(conf=None), 'conf'),
                                    (dict(Bt=-1), 'Bt=-1'), (dict(g=0), 'g=0'), (dict(nb=0), 'nb=0'), (dict(C=-1), 'C=-1'),
                                    (dict(n_frames=0), 'n_frames=0'), (dict(max_boxes=-2), 'max_boxes=-2'),
                                    (dict(C=3), 'cls must be given when C=3'), (dict(margin=float('nan')), 'margin=nan')])
def test_entry_point_refuses_bad_arguments(kw, msg):
    with pytest.raises(_lib.HipExtensionError, match='cy_yolo_decode_tiles_conf: .*' + re.escape(msg)):
        _lib.call('cy_yolo_decode_tiles_conf', *_args(**kw))


def test_entry_point_with_no_tiles_or_no_slots_is_a_no_op():
    nothing = dict(y=None, tile_frame=None, tile_rect=None, frame_hw=None, count=None, dropped=None, image_idx=None, xy=None, conf=None,
                   err=None)
    _lib.call('cy_yolo_decode_tiles_conf', *_args(Bt=0, **nothing))       # nothing is launched
    _lib.call('cy_yolo_decode_tiles_conf', *_args(max_boxes=0, **nothing))
    with pytest.raises(_lib.HipExtensionError, match='g=0'):              # ... but the sizes are still checked
        _lib.call('cy_yolo_decode_tiles_conf', *_args(Bt=0, g=0, **nothing))


# ------------------------------------------------------------------------------------------------ the restatement
HW = [(80, 100)]
INNER = (16, 64, 20, 70)            # a 48 x 50 tile with all four edges inside the frame
G = 2                               # cells of 24 x 25 pixels


def _one_box(cx, cy, w, h, conf=0.9):
    """y [1, 2, 2, 5] whose only box over the threshold has its centre at (cx, cy) and the size (w, h), in tile pixels of INNER."""
    y = np.zeros((1, G, G, 5), np.float32)
    col, row = int(cx // 25), int(cy // 24)
    y[0, row, col] = [conf, (cx - 25 * col) / 25.0, (cy - 24 * row) / 24.0, w / 50.0, h / 48.0]
    return y


# centre and size of a box that violates exactly one side of INNER at margin 2 (corners at x 0.5 / 49.5, y 0.5 / 47.5)
SIDE_BOXES = {'left': (5.5, 24.0, 10.0, 10.0), 'right': (44.5, 24.0, 10.0, 10.0), 'top': (25.0, 5.5, 10.0, 10.0),
              'bottom': (25.0, 42.5, 10.0, 10.0)}
# the same tile pushed against that side of the frame: the edge is the frame's, so it cuts nothing
AT_BORDER = {'left': (16, 64, 0, 50), 'right': (16, 64, 50, 100), 'top': (0, 48, 20, 70), 'bottom': (32, 80, 20, 70)}


@pytest.mark.parametrize('side', R.SIDES)
def test_one_box_per_border_side_is_dropped_and_kept_at_the_frame_border(side):
    y = _one_box(*SIDE_BOXES[side])
    out = R.decode_tiles(y, 0, [0], [INNER], HW, 0.5, 2.0)
    assert (out['count'], out['dropped'], out['err']) == (0, 1, 0)
    assert out['fired'] == dict((s, int(s == side)) for s in R.SIDES)
    kept = R.decode_tiles(y, 0, [0], [AT_BORDER[side]], HW, 0.5, 2.0)
    assert (kept['count'], kept['dropped']) == (1, 0) and kept['idx'].tolist() == [0] and kept['tile'].tolist() == [0]
    cx, cy, w, h = SIDE_BOXES[side]
    y0, _, x0, _ = AT_BORDER[side]
    np.testing.assert_allclose(kept['xy'], [[cx - w / 2 + x0, cy - h / 2 + y0, cx + w / 2 + x0, cy + h / 2 + y0]], rtol=0, atol=1e-5)
    assert kept['conf'].tolist() == [np.float32(0.9)]
    off = R.decode_tiles(y, 0, [0], [INNER], HW, 0.5, -1.0)              # no border rule
    assert (off['count'], off['dropped']) == (1, 0)
    zero = R.decode_tiles(y, 0, [0], [INNER], HW, 0.5, 0.0)              # margin 0: only a box that leaves the tile
    assert (zero['count'], zero['dropped']) == (1, 0)


def test_restatement_edge_cases():
    inside = _one_box(25.0, 24.0, 12.5, 12.0)                            # 0.25 of the tile both ways: exact in float32
    out = R.decode_tiles(inside, 0, [0], [INNER], HW, 0.5, 2.0)
    assert (out['count'], out['dropped']) == (1, 0)
    assert out['xy'].tolist() == [[38.75, 34.0, 51.25, 46.0]]            # (25 -+ 6.25 + 20, 24 -+ 6 + 16)
    nan = inside.copy()
    nan[0, 1, 1, 3] = np.nan                                             # a NaN width: both x corners are NaN, nothing fires
    out = R.decode_tiles(nan, 0, [0], [INNER], HW, 0.5, 2.0)
    assert (out['count'], out['dropped']) == (1, 0) and np.isnan(out['xy'][0, [0, 2]]).all() and out['xy'][0, [1, 3]].tolist() == [34.0, 46.0]
    outside = _one_box(3.0, 24.0, 10.0, 10.0)                            # leaves the tile on the left: dropped at margin 0 too
    assert R.decode_tiles(outside, 0, [0], [INNER], HW, 0.5, 0.0)['dropped'] == 1
    under = _one_box(25.0, 24.0, 10.0, 10.0, conf=0.5)                   # the threshold is strict
    assert R.decode_tiles(under, 0, [0], [INNER], HW, 0.5, 2.0)['count'] == 0
    # bad tiles: a frame index outside the table, an empty rectangle, one that leaves its frame
    for frame, rect in ((1, INNER), (-1, INNER), (0, (16, 16, 20, 70)), (0, (16, 81, 20, 70)), (0, (16, 64, -1, 70))):
        out = R.decode_tiles(inside, 0, [frame], [rect], HW, 0.5, 2.0)
        assert (out['count'], out['dropped'], out['err']) == (0, 0, 1)
    # two frames, classes: (tile, row, column, box) order, the frame as the image index, the first maximum as the class
    y = np.zeros((2, G, G, 13), np.float32)
    y[0, 1, 0, 5:10] = [0.8, 0.5, 0.5, 0.2, 0.2]
    y[0, 1, 0, 10:13] = [0.1, 0.7, 0.7]
    y[1, 0, 1, 0:5] = [0.7, 0.5, 0.5, 0.2, 0.2]
    y[1, 0, 1, 10:13] = [np.nan, 0.2, 0.3]
    out = R.decode_tiles(y, 3, [0, 1], [INNER, (0, 80, 0, 100)], [(80, 100), (80, 100)], 0.5, 2.0)
    assert out['idx'].tolist() == [0, 1] and out['tile'].tolist() == [0, 1] and out['cls'].tolist() == [1, 0]
    assert out['conf'].tolist() == [np.float32(0.8), np.float32(0.7)]


def test_sweep_of_the_restatement_on_a_hand_made_list():
    gt = ([0, 0, 1], [[0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 10]], np.ones(3, np.float32))
    pr = ([0, 1, 1], [[0, 0, 10, 8], [0, 0, 10, 10], [50, 50, 60, 60]], np.array([0.9, 0.4, 0.8], np.float32))
    out = R.confusion_sweep(gt, pr, 2, [0.0, 0.5], [0.5, 0.9])
    assert out[0, 0].tolist() == [2, 1, 1] and out[0, 1].tolist() == [1, 2, 2]
    assert out[1, 0].tolist() == [1, 1, 2] and out[1, 1].tolist() == [0, 2, 3]


# ------------------------------------------------------------------------------------------------ training on the windows
def test_window_labels_visibility_threshold_and_clipped_coordinates():
    window = (10, 58, 20, 70)                                            # 48 x 50
    # 100 x 10 boxes that stick out on the left: 59 and 61 of the 100 columns inside
    out59 = augment.window_labels([[-21.0, 20.0, 79.0, 30.0]], [4], (10, 58, 20, 200), 64, 2, 43)
    assert not out59.any()
    box61 = [[-19.0, 20.0, 81.0, 30.0]]
    y = augment.window_labels(box61, [4], (10, 58, 20, 200), 64, 2, 43)
    want = augment.label_grid([[0.0, 10.0, 61.0, 20.0]], [4], (48, 180), 64, 2, 43, skip_conflicts=False)
    assert y.any() and np.array_equal(y, want) and y[..., 0].sum() == 1 and y[..., 5 + 4].sum() == 1
    # exactly on the threshold counts (at least min_visible), and min_visible is an argument
    on = [[-20.0, 20.0, 30.0, 30.0]]                                     # 30 of 50 columns = 0.6
    assert augment.window_labels(on, [1], (10, 58, 0, 50), 64, 2, 43).any()
    assert not augment.window_labels(on, [1], (10, 58, 0, 50), 64, 2, 43, min_visible=0.7).any()
    # clipped in both directions, relative to the window's origin; a box elsewhere is not labelled; no classes
    boxes = [[60.0, 50.0, 72.0, 60.0], [0.0, 0.0, 10.0, 8.0]]            # 10 x 8 of its 12 x 10 pixels inside
    y = augment.window_labels(boxes, None, window, 64, 2, 0)
    want = augment.label_grid([[40.0, 40.0, 50.0, 48.0]], None, (48, 50), 64, 2, 0, skip_conflicts=False)
    assert np.array_equal(y, want) and y.shape == (2, 2, 5) and y[1, 1, 0] == 1 and y[..., 0].sum() == 1
    assert not augment.window_labels([[5.0, 5.0, 5.0, 9.0]], None, window, 64, 2, 0).any()      # no area


def test_plan_with_tiles_keeps_the_pastes_and_without_tiles_every_bit():
    bank = augment.SignBank(*synth.sign_bank(6, 43, seed=3))
    hw = np.array([[60, 80], [50, 70], [64, 64]])
    bx = [np.array([[10., 5., 30., 25., 1.]]), np.zeros((0, 5)), np.array([[3., 3., 20., 20., 2.], [30., 30., 50., 50., 4.]])]
    spec = TileSpec(2, 2, 8, full=True)
    plain = augment.plan_batch([0, 1, 2], hw, bx, bank, 1, 9, 0, 64, 2, 43)
    same = augment.plan_batch([0, 1, 2], hw, bx, bank, 1, 9, 0, 64, 2, 43, tiles=None)
    for a, b in zip(plain, same):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the plan as it stood before the argument existed: the whole frame, the labels of the pasted boxes
    assert plain[0].tolist() == [[0, 60, 0, 80], [0, 50, 0, 70], [0, 64, 0, 64]] and plain[1].tolist() == [0, 2, 3, 6]
    for k in range(3):
        rows, boxes, classes = augment.plan_pastes(augment.sample_rng(9, k, 0), bx[k][:, 0:4], hw[k], bank, 1)
        assert np.array_equal(plain[2][plain[1][k]:plain[1][k + 1]], rows)
        assert np.array_equal(plain[3][k], augment.label_grid(boxes, classes, hw[k], 64, 2, 43, skip_conflicts=False))
    rect, begin, rows, y = augment.plan_batch([0, 1, 2], hw, bx, bank, 1, 9, 0, 64, 2, 43, tiles=spec)
    assert np.array_equal(begin, plain[1]) and np.array_equal(rows, plain[2])            # the same pastes
    picks = []
    for k in range(3):
        rng = augment.sample_rng(9, k, 0)
        _, boxes, classes = augment.plan_pastes(rng, bx[k][:, 0:4], hw[k], bank, 1)
        table = spec.rects(*hw[k])
        pick = int(rng.integers(0, 5))                                   # one more draw, behind the sample's paste draws
        picks.append(pick)
        assert rect[k].tolist() == table[pick].tolist()
        assert np.array_equal(y[k], augment.window_labels(boxes, classes, table[pick], 64, 2, 43))
    print('windows drawn: %s' % picks)
    assert len(set(picks)) > 1
    other = augment.plan_batch([0, 1, 2], hw, bx, bank, 1, 9, 1, 64, 2, 43, tiles=spec)   # another iteration: other draws
    assert not np.array_equal(other[2], rows)


# ------------------------------------------------------------------------------------------------ the streaming detector
def test_sign_detector_refuses_tiles_before_any_device_work():
    dp = types.SimpleNamespace(n_classes=0, n_grid=13, n_boxes=3, darknet_input=416, capsule_input=32)
    with pytest.raises(ValueError, match='tiles need nms_iou'):
        serve.SignDetector(None, dp, None, None, tiles=TileSpec(2, 3, 128))
    with pytest.raises(ValueError, match='3549 candidates per frame, the suppression step holds 3413'):
        serve.SignDetector(None, dp, None, None, nms_iou=0.45, tiles=TileSpec(2, 3, 128, full=True))
    with pytest.raises(ValueError, match='must be a TileSpec'):
        serve.SignDetector(None, dp, None, None, nms_iou=0.45, tiles=(2, 3, 128))


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_arguments_and_refusals():
    import importlib.util
    spec = importlib.util.spec_from_file_location('cy_main_tiles_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    a = m.parser.parse_args([])
    assert a.tiles is None and a.tile_overlap is None and a.tile_full is False and a.tile_margin is None
    m.check_tiles(a)
    assert a.tile_spec is None
    serve_argv = ['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last']
    a = m.parser.parse_args(serve_argv + ['--nms', '0.45', '--tiles', '2x3', '--tile_overlap', '128', '--tile_full', '--tile_margin', '-1'])
    m.check_tiles(a)
    assert a.tile_spec == TileSpec(2, 3, 128, True, -1.0)
    a = m.parser.parse_args(['--mode', 'detect', '--model', 'darknet_r', '--restore', 'last', '--nms', '0.5', '--tiles', '1x1'])
    m.check_tiles(a)
    assert a.tile_spec == TileSpec(1, 1, 0, False, 2.0)
    a = m.parser.parse_args(['--mode', 'train', '--model', 'darknet_d', '--augment', '--tiles', '2x2', '--tile_overlap', '8'])
    m.check_tiles(a)
    assert a.tile_spec == TileSpec(2, 2, 8)
    for argv, msg in ((serve_argv + ['--tiles', '2x3'], '--tiles needs --nms'),
                      (serve_argv + ['--nms', '0.45', '--tile_overlap', '8'], '--tile_overlap belongs to the tiling'),
                      (serve_argv + ['--nms', '0.45', '--tile_full'], '--tile_full belongs to the tiling'),
                      (serve_argv + ['--nms', '0.45', '--tile_margin', '1'], '--tile_margin belongs to the tiling'),
                      (serve_argv + ['--nms', '0.45', '--tiles', '2by3'], '--tiles 2by3'),
                      (serve_argv + ['--nms', '0.45', '--tiles', '2x3', '--tile_overlap', '-4'], '--tiles 2x3'),
                      (['--mode', 'train', '--model', 'darknet_d', '--tiles', '2x3'], '--tiles runs the detector on windows'),
                      (['--mode', 'train', '--model', 'darkcapsule', '--augment', '--tiles', '2x3'], 'decodes into boxes'),
                      (['--mode', 'predict', '--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last', '--nms', '0.45',
                        '--tiles', '2x3'], '--tiles runs the detector on windows')):
        with pytest.raises(SystemExit, match=re.escape(msg)):
            m.main(argv)

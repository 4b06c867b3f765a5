"""Host-side tests of the sign-paste augmentation and the data-set builder (no GPU): the label arithmetic against what the reference's
own functions returned (tests/golden/builddata.npz), the integer resize rule of tests/augment_ref.py against the float64 yardstick,
the paste plan, the parsers, and the C-ABI's new symbol."""
import importlib.util
import os
import re

import numpy as np
import pytest

from helpers import REPO, load_golden

from capsyolo_amd import _lib, augment, build_data, interpret, synth
from augment_ref import composite, resize_int
from pipeline_ref import crop_resize

FRAME_SIZES = [(37, 53), (64, 48), (48, 48), (90, 33), (33, 90)]
OUT_SIZES = [(32, 32), (96, 96), (40, 56)]


def _bank(n=6, seed=3):
    return augment.SignBank(*synth.sign_bank(n, 43, seed=seed))


# ---------------------------------------------------------------- label arithmetic against the reference

def test_box_arithmetic_matches_the_reference_to_the_last_bit():
    g = load_golden('builddata')
    assert len(g['box_xy']) >= 40
    for k in range(len(g['box_xy'])):
        resized, cwh, norm, pos = augment.box_to_cell(g['box_xy'][k], g['box_hw'][k], int(g['box_side'][k]), int(g['box_grid'][k]))
        assert np.array_equal(np.array(resized), g['box_resized'][k]), k
        assert np.array_equal(np.array(cwh), g['box_cwh'][k]), k
        assert np.array_equal(np.array(norm), g['box_norm'][k]), k
        assert tuple(pos) == tuple(g['box_pos'][k]), k
    assert (g['box_norm'][:, 0:2] == 0.0).any()                      # centres exactly on a cell boundary are among them


@pytest.mark.parametrize('k', [0, 1, 2])
def test_label_grid_matches_the_reference_grids(k):
    g = load_golden('builddata')
    boxes = g['grid%d_boxes' % k]
    conflicts = []
    y = augment.label_grid(boxes[:, 0:4], boxes[:, 4], g['grid%d_hw' % k], int(g['grid%d_side' % k]), int(g['grid%d_g' % k]), 43,
                           skip_conflicts=not bool(g['grid%d_overwrite' % k]), conflicts=conflicts)
    assert y.dtype == np.float64 and np.array_equal(y, g['grid%d_y' % k])
    if not g['grid%d_overwrite' % k]:
        assert len(conflicts) == int(g['grid%d_conflicts' % k])


def test_overwrite_keeps_the_earlier_class_bit():
    boxes = np.array([[10., 10., 30., 30.], [12., 14., 36., 40.]])
    cls = [5, 7]
    y = augment.label_grid(boxes, cls, (97, 131), 64, 2, 43, skip_conflicts=False)
    second = augment.label_grid(boxes[1:], cls[1:], (97, 131), 64, 2, 43, skip_conflicts=False)
    assert np.array_equal(y[0, 0, 0:5], second[0, 0, 0:5])           # the later box's five numbers
    assert y[0, 0, 5 + 5] == 1 and y[0, 0, 5 + 7] == 1 and y[0, 0, 5:].sum() == 2      # ... and BOTH class bits, like the reference
    conflicts = []
    plain = augment.label_grid(boxes, cls, (97, 131), 64, 2, 43, skip_conflicts=True, conflicts=conflicts)
    first = augment.label_grid(boxes[:1], cls[:1], (97, 131), 64, 2, 43, skip_conflicts=True)
    assert np.array_equal(plain, first) and conflicts == [1]
    with pytest.raises(ValueError):
        augment.label_grid([[200., 10., 240., 30.]], [0], (97, 131), 64, 2, 43, True)


# ---------------------------------------------------------------- the integer resize rule

@pytest.mark.parametrize('oh,ow', OUT_SIZES)
def test_integer_rule_is_within_half_a_level_of_the_float_yardstick(oh, ow):
    rng = np.random.default_rng(7)
    for h, w in FRAME_SIZES:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = resize_int(im, oh, ow)
        want = crop_resize(im, (0, h, 0, w), oh, ow)
        assert got.dtype == np.uint8 and np.abs(got.astype(np.float64) - want).max() <= 0.5 + 1e-9, (h, w)


def test_integer_rule_is_the_identity_at_equal_size():
    rng = np.random.default_rng(8)
    for h, w in FRAME_SIZES:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(resize_int(im, h, w), im)
    # so a sign pasted 1:1 is a plain copy of its ROI
    frame, sign = np.zeros((20, 20, 3), np.uint8), rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    out = composite(frame, [sign], [[0, 1, 8, 2, 6, 5, 12, 3, 7]])
    assert np.array_equal(out[5:12, 3:7], sign[1:8, 2:6]) and out.sum() == sign[1:8, 2:6].sum()


# ---------------------------------------------------------------- the paste plan

def test_plan_existing_boxes_first_then_additions_inside_the_frame():
    bank = _bank()
    hw = (60, 80)
    boxes = np.array([[10.7, 5.2, 30.9, 25.1], [40.0, 30.0, 52.5, 44.9]])
    rows, lab, cls = augment.plan_pastes(augment.sample_rng(0, 3, 0), boxes, hw, bank, add_signs=3)
    assert rows.shape == (5, 9) and rows.dtype == np.int32 and lab.shape == (5, 4) and cls.shape == (5,)
    # the existing boxes, corners truncated, in their order; the label is the truncated box with the sign's class
    assert rows[0, 5:9].tolist() == [5, 25, 10, 30] and rows[1, 5:9].tolist() == [30, 44, 40, 52]
    assert lab[0].tolist() == [10, 5, 30, 25] and lab[1].tolist() == [40, 30, 52, 44]
    for r, b, c in zip(rows, lab, cls):
        s = int(r[0])
        assert r[1:5].tolist() == bank.rois[s].tolist() and c == bank.classes[s]
        assert 0 <= r[5] < r[6] <= hw[0] and 0 <= r[7] < r[8] <= hw[1]
        assert b.tolist() == [r[7], r[5], r[8], r[6]]
    for r in rows[2:]:                                                # additions are 1:1 copies and the whole sign image fits
        s = int(r[0])
        assert r[6] - r[5] == r[2] - r[1] and r[8] - r[7] == r[4] - r[3]
        assert r[5] + bank.hw[s, 0] <= hw[0] and r[7] + bank.hw[s, 1] <= hw[1]


def test_plan_is_determined_by_seed_sample_iteration():
    bank = _bank()
    boxes = np.array([[10., 5., 30., 25.]])
    plan = lambda *key: augment.plan_pastes(augment.sample_rng(*key), boxes, (60, 80), bank, 2)[0]
    assert np.array_equal(plan(1, 4, 0), plan(1, 4, 0))
    others = [plan(2, 4, 0), plan(1, 5, 0), plan(1, 4, 1)]
    assert all(not np.array_equal(plan(1, 4, 0), o) for o in others)
    # a batch plan is the samples' own plans, whatever else is in the batch
    hw = np.array([(60, 80), (50, 70), (64, 64)])
    bx = [np.array([[10., 5., 30., 25., 1.]]), np.zeros((0, 5)), np.array([[5., 5., 20., 20., 2.], [30., 30., 50., 60., 3.]])]
    rect, begin, rows, y = augment.plan_batch([0, 1, 2], hw, bx, bank, 1, 9, 0, 64, 2, 43)
    assert begin.tolist() == [0, 2, 3, 6] and rect.tolist() == [[0, 60, 0, 80], [0, 50, 0, 70], [0, 64, 0, 64]] and y.shape == (3, 2, 2, 48)
    _, b2, rows2, y2 = augment.plan_batch([2], hw[2:], bx[2:], bank, 1, 9, 0, 64, 2, 43)
    assert np.array_equal(rows2, rows[3:6]) and np.array_equal(y2[0], y[2])


def test_plan_refuses_degenerate_boxes():
    bank = _bank()
    rng = augment.sample_rng(0, 0, 0)
    for bad in ([10.2, 5.0, 10.9, 25.0], [10.0, 5.9, 30.0, 5.95], [30.0, 5.0, 10.0, 25.0], [-3.0, 5.0, 10.0, 25.0], [70.0, 5.0, 81.0, 25.0],
                [np.nan, 5.0, 10.0, 25.0]):
        with pytest.raises(ValueError):
            augment.plan_pastes(rng, np.array([bad]), (60, 80), bank, 0)
    with pytest.raises(ValueError):                                   # no sign of this bank fits into a 10 x 10 frame
        augment.plan_pastes(rng, np.zeros((0, 4)), (10, 10), bank, 1)
    with pytest.raises(ValueError):
        augment.plan_pastes(rng, np.zeros((0, 4)), (60, 80), bank, augment.MAX_PASTES + 1)
    with pytest.raises(ValueError):
        augment.SignBank([np.zeros((9, 7, 3), np.uint8)], [[0, 10, 0, 7]], [0])


def test_synthetic_boxes_and_bank():
    frames = synth.raw_images(5)
    boxes = synth.raw_boxes(frames)
    again = synth.raw_boxes(synth.raw_images(2, first=3), first=3)
    assert np.array_equal(boxes[3], again[0]) and np.array_equal(boxes[4], again[1])
    bank = _bank(8)
    for im, b in zip(frames, boxes):
        assert b.ndim == 2 and b.shape[1] == 5 and 1 <= len(b) <= 3
        augment.plan_pastes(augment.sample_rng(0, 0, 0), b[:, 0:4], im.shape[0:2], bank, 2)       # non-degenerate, and signs fit
    assert (bank.rois[:, 0] > 0).all() and (bank.rois[:, 1] < bank.hw[:, 0]).all()


# ---------------------------------------------------------------- parsers

def test_parsers_on_files_written_here(tmp_path):
    rng = np.random.default_rng(5)
    im = rng.integers(0, 256, (11, 13, 3), dtype=np.uint8)
    interpret.write_ppm(str(tmp_path / 'a.ppm'), im)
    assert np.array_equal(interpret.read_ppm(str(tmp_path / 'a.ppm')), im)
    (tmp_path / 'gt.txt').write_text('00000.ppm;774;411;815;446;11\n00001.ppm;983;388;1024;432;40\n00000.ppm;10;20;30;40;2\n\n')
    gt = build_data.read_gt(str(tmp_path / 'gt.txt'))
    assert list(gt) == ['00000.ppm', '00001.ppm']
    assert gt['00000.ppm'].tolist() == [[774, 411, 815, 446, 11], [10, 20, 30, 40, 2]] and gt['00000.ppm'].dtype == np.float64
    (tmp_path / 'bad.txt').write_text('00000.ppm;1;2;3\n')
    with pytest.raises(ValueError):
        build_data.read_gt(str(tmp_path / 'bad.txt'))
    root = tmp_path / 'GTSRB'
    for c in (0, 1):
        d = root / 'Images' / ('%05d' % c)
        d.mkdir(parents=True)
        lines = ['Filename;Width;Height;Roi.X1;Roi.Y1;Roi.X2;Roi.Y2;ClassId']
        for k in range(2):
            h, w = 10 + k + c, 12 + 2 * k
            interpret.write_ppm(str(d / ('%05d_%05d.ppm' % (c, k))), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            lines.append('%05d_%05d.ppm;%d;%d;2;1;%d;%d;%d' % (c, k, w, h, w - 2, h - 1, c))
        (d / ('GT-%05d.csv' % c)).write_text('\n'.join(lines) + '\n')
    names, rois, classes, sizes = build_data.read_sign_csv(str(root / 'Images' / '00001' / 'GT-00001.csv'))
    assert names == ['00001_00000.ppm', '00001_00001.ppm'] and rois.tolist() == [[1, 10, 2, 10], [1, 11, 2, 12]]
    assert classes.tolist() == [1, 1] and sizes.tolist() == [[11, 12], [12, 14]]
    images, rois, classes, first = build_data.read_gtsrb(str(root))
    assert len(images) == 4 and first == [0, 2, 4] and classes.tolist() == [0, 0, 1, 1] and images[3].shape == (12, 14, 3)
    bank = build_data.load_bank(str(root))
    assert bank.n == 4 and bank.hw.tolist() == [[10, 12], [11, 14], [11, 12], [12, 14]]
    readme = ['line %d' % i for i in range(39)] + ['0 = speed limit 20 (prohibitory)', '1 = speed limit 30 (prohibitory)', '']
    (tmp_path / 'Readme.txt').write_text('\n'.join(readme))
    assert build_data.read_class_names(str(tmp_path / 'Readme.txt')) == [' speed limit 20 (prohibitory)', ' speed limit 30 (prohibitory)']


# ---------------------------------------------------------------- C-ABI and command line

def test_cabi_exports_the_paste_kernel():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    assert re.search(r'\bint\s+cy_paste_resize_u8\s*\(', header)
    lib = _lib.load()
    assert 'cy_paste_resize_u8' in _lib.EXPORTS and hasattr(lib, 'cy_paste_resize_u8')
    assert len(_lib._SIGS['cy_paste_resize_u8']) == 22
    assert augment.kernel_max_pastes() == augment.MAX_PASTES == 64
    null = [None, None, None, 1, 1, None, None, None, 0, 0, None, None, None]
    _lib.call('cy_paste_resize_u8', *(null + [0, None, 0, 8, 8, 0, None, None, None]))       # n = 0 is valid and launches nothing
    with pytest.raises(_lib.HipExtensionError, match='null argument'):
        _lib.call('cy_paste_resize_u8', *(null + [1, None, 0, 8, 8, 0, None, None, None]))


def test_commands_accept_the_new_arguments():
    spec = importlib.util.spec_from_file_location('cy_main_augment_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    args = m.parser.parse_args(['--model', 'darknet_d', '--augment', '--gtsrb', '/x'])
    assert args.augment is True and args.gtsrb == '/x' and m.parser.parse_args([]).augment is False
    assert callable(m.augmented_data) and '--augment' in m.__doc__
    spec = importlib.util.spec_from_file_location('cy_build_data_host', os.path.join(REPO, 'build_data.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    a = b.parser.parse_args(['--aug', '2', '--root', 'r', '--gtsrb', 'g', '--seed', '3', '--keep_raw'])
    assert (a.aug, a.root, a.gtsrb, a.seed, a.keep_raw) == (2, 'r', 'g', 3, True)

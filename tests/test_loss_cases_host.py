"""CPU tests of the loss case table (tests/loss_cases.py): what makes tests/test_gpu_losses.py mean something.
(a) every case keeps the conditions it was made for, computed in fp64; (b) the reference alone passes: the oracle in fp32 is
accepted against the oracle in fp64 on every case; (c) the cases catch wrong kernels: mutants of the oracle (fp32, each a
plausible kernel bug) are rejected by `compare`, each on a case that is named."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as L
from oracle import loss_fns as OL

T = torch.from_numpy
DARK = L.names('dark')
DENSE_19 = [n for n in DARK if '3x19' in n]
DENSE = DENSE_19 + ['dark/2x4_nb4_c3']


# ------------------------------------------------------------------------------------------------ (a) the conditions
def _iou64(case):
    """(object mask [cells], IoU [cells, n_boxes]) of a dark_loss case in fp64, by the oracle's own functions."""
    p, inp = case['params'], case['inputs']
    nb, g = p['n_boxes'], p['n_grid']
    yp, yt = T(inp['y_pred']), T(inp['y_true'])
    boxes = yp[..., :5 * nb].reshape(yp.shape[:3] + (nb, 5))
    iou = OL.iou_xyxy(OL.cwh_to_xyxy(boxes[..., 1:5], p['darknet_input'], g), OL.cwh_to_xyxy(yt[..., None, 1:5], p['darknet_input'], g))
    return (yt[..., 0] == 1).reshape(-1).numpy(), iou.reshape(-1, nb).numpy()


@pytest.mark.parametrize('name', DARK)
def test_dark_cases_shapes_and_iou_gaps(name):
    case = L.CASES[name]
    p, inp = case['params'], case['inputs']
    nb, C, g = p['n_boxes'], p['n_classes'], p['n_grid']
    B = inp['y_pred'].shape[0]
    assert inp['y_pred'].shape == (B, g, g, 5 * nb + C) and inp['y_true'].shape[:3] == (B, g, g)
    assert inp['y_true'].shape[3] == (48 if name == 'dark/wide_labels' else 5 + C)
    for a in inp.values():                                               # float64 holding float32-representable values
        assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
    obj, iou = _iou64(case)
    assert np.isfinite(iou[obj]).all()
    if nb > 1 and obj.any():
        top = np.sort(iou[obj], axis=1)[:, ::-1]
        gap = top[:, 0] - top[:, 1]
        tie = top[:, 0] == top[:, 1]
        # an fp32 IoU is about 1e-7 off: with a gap of 1e-5 (or the same bits) no rounding changes which box is responsible
        assert (tie | (gap >= 1e-5)).all(), 'smallest IoU gap %.3g' % gap[~tie].min()
        if name in DENSE:
            assert not tie.any()
            print('%s: smallest gap between the best and the second IoU %.3g' % (name, gap.min()))


@pytest.mark.parametrize('name', DENSE)
def test_dense_dark_cases_use_every_box_position(name):
    case = L.CASES[name]
    obj, iou = _iou64(case)
    counts = np.bincount(iou[obj].argmax(1), minlength=case['params']['n_boxes'])
    assert (counts >= 1).all(), counts
    first = case['inputs']['y_true'][..., 0]
    assert 0.3 < (first == 1).mean() < 0.7 and ((first == 0) | (first == 1)).all()


@pytest.mark.parametrize('name', DENSE_19)
def test_grid_19_cases_need_a_second_pass(name):
    yp = L.CASES[name]['inputs']['y_pred']
    cells = yp.shape[0] * yp.shape[1] * yp.shape[2]
    assert cells == 1083 and cells > L.LT and cells % L.LT == 59
    obj, _ = _iou64(L.CASES[name])
    assert obj[L.LT:].any() and (~obj[L.LT:]).any()                     # objects and empty cells in the second pass


def test_hand_built_case_contains_its_four_situations():
    case = L.CASES['dark/hand_built']
    obj, iou = _iou64(case)
    yp, yt = case['inputs']['y_pred'].reshape(4, 10), case['inputs']['y_true'].reshape(4, 5)
    assert obj.tolist() == [True, True, False, True] and not (yt[:, 0] == 0).any()       # and no empty cell in the batch
    assert iou[0, 0] == iou[0, 1] > 0.1 and yp[0, 0] != yp[0, 5]         # the same bits; the confidences tell the boxes apart
    assert iou[1, 0] == 0.0 and iou[1, 1] == 0.0 and yp[1, 0] != yp[1, 5]
    assert yt[2, 0] == 0.5
    assert iou[3, 1] > iou[3, 0] + 0.1
    # the same in fp32, as the kernel computes it
    p = case['params']
    boxes = T(yp).float().reshape(4, 2, 5)
    iou32 = OL.iou_xyxy(OL.cwh_to_xyxy(boxes[..., 1:5], p['darknet_input'], 2), OL.cwh_to_xyxy(T(yt).float()[:, None, 1:5], p['darknet_input'], 2))
    assert iou32[0, 0] == iou32[0, 1] and (iou32[1] == 0).all()
    ref = L.reference('dark/hand_built')
    assert not ref['grad']['y_pred'].reshape(4, 10)[2].any()             # cell 2: a gradient of exactly zero
    g = ref['grad']['y_pred'].reshape(4, 10)
    assert g[0, 1:5].any() and not g[0, 6:10].any() and g[1, 1:5].any() and not g[1, 6:10].any() and g[3, 6:10].any() and not g[3, 1:5].any()
    assert g[1, 0] == 2.0 * yp[1, 0]                                     # box 0 of cell 1: confidence target 0, batch of one


def test_special_dark_cases():
    assert (L.CASES['dark/all_objects']['inputs']['y_true'][..., 0] == 1).all()
    assert not L.CASES['dark/no_object']['inputs']['y_true'].any()
    ref = L.reference('dark/no_object')
    assert np.isnan(ref['avg_iou']) and np.isfinite(ref['loss']) and ref['loss'] > 0 and np.isfinite(ref['grad']['y_pred']).all()
    # the wide labels: the oracle reads the first five columns only, and class columns are set behind them
    wide = L.CASES['dark/wide_labels']
    assert wide['params']['n_classes'] == 0 and wide['inputs']['y_true'].shape[-1] == 48 and wide['inputs']['y_true'][..., 5:].any()
    narrow = dict(wide, inputs=dict(wide['inputs'], y_true=np.ascontiguousarray(wide['inputs']['y_true'][..., :5])))
    a, b = L.reference('dark/wide_labels'), L.run(narrow, OL)
    assert a['loss'] == b['loss'] and np.array_equal(a['grad']['y_pred'], b['grad']['y_pred'])


def test_capsule_kind_cases():
    for name in L.names('darkcapsule') + L.names('darkcapsule2') + L.names('darkcapsule3'):
        first = L.CASES[name]['inputs']['y'][..., 0]
        if first.size > 100:
            assert all((first == v).mean() > 0.1 for v in (0.0, 0.5, 1.0)), name      # empty, fractional and object cells
    assert L.CASES['darkcapsule/3x19_w5']['inputs']['y'].shape[-1] == 5 and L.CASES['darkcapsule/3x19_w48']['inputs']['y'].shape[-1] == 48
    c3 = L.CASES['darkcapsule3/3x19_c43_d21']['inputs']['caps']
    assert c3.shape == (3, 19, 19, 43, 21) and 46000 < c3.size // 21 < 47000
    assert L.CASES['darkcapsule3/3x19_c1_d9']['inputs']['caps'].shape == (3, 19, 19, 1, 9)
    # the zero capsule: a finite loss, NaN in that cell's gradient and nowhere else
    ref = L.reference('darkcapsule/zero_capsule')
    nan = np.isnan(ref['grad']['caps']).reshape(8, 5)
    assert np.isfinite(ref['loss']) and nan[1].all() and not np.delete(nan, 1, 0).any()
    for name in L.names('capsule'):
        c = L.CASES[name]
        y, C = c['inputs']['y'], c['params']['n_classes']
        assert y.min() == 0 and y.max() == C - 1
    assert L.CASES['capsule/25x43']['inputs']['scores'].size == 1075 > L.LT
    assert L.CASES['capsule/5x43_recon']['inputs']['recon'].shape == (5, 3, 32, 32)
    for kind in L.FN:                                                    # every loss has its three ways of being called
        mine = [L.CASES[n] for n in L.names(kind)]
        assert any(c.get('scale') == -1.5 for c in mine) and any('extra' in c for c in mine) and any('permute' in c for c in mine)


# ------------------------------------------------------------------------------------------------ (b) the reference alone passes
@pytest.mark.parametrize('name', L.names())
def test_oracle_fp32_passes(name):
    case = L.CASES[name]
    fr = L.compare(case['kind'], L.run(case, OL, torch.float32), L.reference(name))
    print(name, dict((k, '%.3g' % v) for k, v in fr.items()))
    assert max(fr.values()) < 0.05          # the reference's own fp32 rounding uses a few per cent of the tolerance at the most


# ------------------------------------------------------------------------------------------------ (c) mutants
def dark_loss_switched(y_pred, y_true, params, last_max=False, drop_not_responsible=False, attach_iou=False, max_cells=None,
                       short_stride=False):
    """oracle.loss_fns.dark_loss restated with one switch per kernel bug; with no switch set it is the oracle (tested below)."""
    nb, C = params.n_boxes, params.n_classes
    Bt, g = y_true.shape[0], y_true.shape[1]
    y_true = y_true.to(y_pred.dtype)
    if short_stride:                                                     # the label buffer walked with 5 + n_classes, whatever its rows are
        y_true = y_true.reshape(-1)[:Bt * g * g * (5 + C)].reshape(Bt, g, g, 5 + C)
    boxes = y_pred[..., :5 * nb].reshape(Bt, g, g, nb, 5)
    tbox = y_true[..., :5]
    live = torch.ones(Bt * g * g, dtype=y_pred.dtype)
    if max_cells is not None:
        live[max_cells:] = 0
    live = live.reshape(Bt, g, g)
    obj = (tbox[..., 0] == 1).to(y_pred.dtype) * live
    noobj = (tbox[..., 0] == 0).to(y_pred.dtype) * live

    def corners(cwh):
        out = OL.cwh_to_xyxy(cwh, params.darknet_input, g)
        if attach_iou:
            cell = 1.0 * params.darknet_input / g
            hw, hh = cwh[..., 2] * params.darknet_input / 2, cwh[..., 3] * params.darknet_input / 2
            out = torch.stack([cwh[..., 0] * cell - hw, cwh[..., 1] * cell - hh, cwh[..., 0] * cell + hw, cwh[..., 1] * cell + hh], dim=-1)
        return out
    pc = boxes[..., 0]
    iou = OL.iou_xyxy(corners(boxes[..., 1:5]), corners(tbox[..., None, 1:5]))
    iou = torch.where(obj[..., None] > 0, iou, torch.zeros_like(iou))
    best_iou, best = iou.max(dim=-1)
    if last_max:
        best = nb - 1 - iou.flip(-1).argmax(dim=-1)
    if not attach_iou:
        best_iou = best_iou.detach()
    resp = F.one_hot(best, nb).to(y_pred.dtype)
    noobj_pc = (noobj[..., None] * pc ** 2).sum()
    if not drop_not_responsible:
        noobj_pc = noobj_pc + (obj[..., None] * (1 - resp) * pc ** 2).sum()
    obj_pc = (obj[..., None] * resp * (pc - best_iou[..., None]) ** 2).sum()
    obj_xy = (obj[..., None, None] * resp[..., None] * (boxes[..., 1:3] - tbox[..., None, 1:3]) ** 2).sum()
    sel = (obj[..., None] * resp)[..., None]
    safe_wh = torch.where(sel > 0, boxes[..., 3:5], torch.ones_like(boxes[..., 3:5]))
    safe_t = torch.where(obj[..., None] > 0, tbox[..., 3:5], torch.ones_like(tbox[..., 3:5]))
    obj_wh = (sel * (safe_wh.sqrt() - safe_t[..., None, :].sqrt()) ** 2).sum()
    obj_cls = 0.0
    if C != 0:
        obj_cls = (obj[..., None] * (y_true[..., 5:] - y_pred[..., 5 * nb:]) ** 2).sum()
    loss = (params.l_coord * obj_xy + params.l_coord * obj_wh + obj_pc + params.l_noobj * noobj_pc + obj_cls) / Bt
    return loss, ((obj * best_iou).sum() / obj.sum()).detach()


_POLAR = OL.polar_transform


def _polar_swapped(t):
    """polar_transform with the w and h angles exchanged: (x pi, y pi, w pi, h 2 pi)."""
    r, x, y, w, h = t.unbind(-1)
    return _POLAR(torch.stack([r, x, y, h, w], dim=-1))


def _with_polar(fn_name, polar):
    def fn(*args, **kw):
        saved = OL.polar_transform
        OL.polar_transform = polar
        try:
            return getattr(OL, fn_name)(*args, **kw)
        finally:
            OL.polar_transform = saved
    return fn


def _first_cells(fn_name, width_of):
    """The loss over the first 1024 cells (items) only: a kernel whose threads make one pass."""
    def fn(a, y, params, *rest):
        B = a.shape[0]
        if fn_name == 'capsule_loss':                                    # items are (row, class) pairs
            onehot = F.one_hot(y, params.n_classes).to(a.dtype).reshape(-1)[:L.LT]
            return OL.margin_terms(a.reshape(-1)[:L.LT], onehot).sum() / B
        w = width_of(a)
        return getattr(OL, fn_name)(a.reshape(1, -1, w)[:, :L.LT], y.reshape(1, -1, y.shape[-1])[:, :L.LT], params) / B
    return fn


def _gradient_over_sqrt2(fn_name):
    """The value of the oracle, its gradient divided by sqrt(2): the scaling of the capsules applied once in the backward."""
    def fn(caps, y, params):
        full = getattr(OL, fn_name)(caps, y, params)
        return full.detach() + (full - full.detach()) / math.sqrt(2)
    return fn


def _darkcapsule3_label_without_y_r(caps, y, params):
    y = y.to(caps.dtype)
    caps = caps * math.sqrt(2)
    y_r, y_phi = OL.polar_transform(y[..., :5])
    cap_r = (caps[..., 5:] ** 2).sum(dim=-1) ** 0.5
    return (OL.margin_terms(cap_r, y[..., 5:]).sum() - (caps[..., :5] * y_phi.unsqueeze(3)).sum()) / y.shape[0]


def _mod(**fns):
    return types.SimpleNamespace(**fns)


def _dark_mod(**switch):
    return _mod(dark_loss=lambda yp, yt, p: dark_loss_switched(yp, yt, p, **switch))


# mutant -> (module, the case that must reject it)
MUTANTS = {
    'last maximum wins': (_dark_mod(last_max=True), 'dark/hand_built'),
    'not-responsible confidence term dropped': (_dark_mod(drop_not_responsible=True), 'dark/3x19_nb4_c43'),
    'not-responsible confidence term dropped, one cell': (_dark_mod(drop_not_responsible=True), 'dark/one_cell'),
    'IoU not detached': (_dark_mod(attach_iou=True), 'dark/3x19_nb2_c0'),
    'IoU not detached, small': (_dark_mod(attach_iou=True), 'dark/2x4_nb4_c3'),
    'dark_loss: cells past 1024 ignored': (_dark_mod(max_cells=L.LT), 'dark/3x19_nb1_c0'),
    'dark_loss: labels strided by 5 + n_classes': (_dark_mod(short_stride=True), 'dark/wide_labels'),
    'darkcapsule: w and h angles swapped': (_mod(darkcapsule_loss=_with_polar('darkcapsule_loss', _polar_swapped)), 'darkcapsule/2x2_w5'),
    'darkcapsule2: w and h angles swapped': (_mod(darkcapsule2_loss=_with_polar('darkcapsule2_loss', _polar_swapped)), 'darkcapsule2/2x2_c3'),
    'darkcapsule3: w and h angles swapped': (_mod(darkcapsule3_loss=_with_polar('darkcapsule3_loss', _polar_swapped)), 'darkcapsule3/2x2_c1_d21'),
    'darkcapsule: cells past 1024 ignored': (_mod(darkcapsule_loss=_first_cells('darkcapsule_loss', lambda a: 5)), 'darkcapsule/3x19_w48'),
    'darkcapsule2: cells past 1024 ignored': (_mod(darkcapsule2_loss=_first_cells('darkcapsule2_loss', lambda a: a.shape[-1])),
                                              'darkcapsule2/3x19_c43'),
    'capsule: items past 1024 ignored': (_mod(capsule_loss=_first_cells('capsule_loss', None)), 'capsule/25x43'),
    'darkcapsule: labels strided by 5': (_mod(darkcapsule_loss=lambda c, y, p: OL.darkcapsule_loss(
        c, y.reshape(-1)[:c.numel()].reshape(c.shape), p)), 'darkcapsule/2x2_w8'),
    'darkcapsule2: sqrt(2) once in the gradient': (_mod(darkcapsule2_loss=_gradient_over_sqrt2('darkcapsule2_loss')), 'darkcapsule2/2x2_c3'),
    'darkcapsule3: sqrt(2) once in the gradient': (_mod(darkcapsule3_loss=_gradient_over_sqrt2('darkcapsule3_loss')), 'darkcapsule3/2x2_c3_d9'),
    'darkcapsule3: margin label without y_r': (_mod(darkcapsule3_loss=_darkcapsule3_label_without_y_r), 'darkcapsule3/2x2_c3_d21'),
}


def test_unswitched_restatement_is_the_oracle():
    """The mutants differ from the oracle by their switch alone: without one, the restatement gives the oracle's bits."""
    for name in DARK:
        a = L.run(L.CASES[name], _dark_mod(), torch.float32)
        b = L.run(L.CASES[name], OL, torch.float32)
        assert a['loss'] == b['loss'] and np.array_equal(a['avg_iou'], b['avg_iou'], equal_nan=True), name
        assert np.array_equal(a['grad']['y_pred'], b['grad']['y_pred']), name
    c = L.CASES['darkcapsule3/2x2_c3_d21']
    same = _mod(darkcapsule3_loss=_with_polar('darkcapsule3_loss', _POLAR))
    assert np.array_equal(L.run(c, same, torch.float32)['grad']['caps'], L.run(c, OL, torch.float32)['grad']['caps'])


@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_mutant_is_rejected(mutant):
    module, name = MUTANTS[mutant]
    case = L.CASES[name]
    got = L.run(case, module, torch.float32)
    fr = L.fractions(case['kind'], got, L.reference(name))
    print(mutant, name, dict((k, '%.3g' % v) for k, v in fr.items()))
    assert not L.accepts(case['kind'], got, L.reference(name)), 'the mutant "%s" is not rejected by the case %s' % (mutant, name)
    # and by a wide margin: an error a hundred times the reference's own fp32 rounding, not one at the edge of the tolerance
    assert max(fr.values()) > 5.0, 'the mutant "%s" misses the tolerance of the case %s only narrowly: %s' % (mutant, name, fr)

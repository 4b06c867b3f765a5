"""The cases of the loss tests: one table, shared by tests/test_loss_cases_host.py (which checks on the CPU that every case keeps
its conditions, that the reference alone passes and that wrong kernels are caught) and tests/test_gpu_losses.py (which runs
csrc/loss.hip on them).  The yardstick is oracle/loss_fns.py in torch.float64 on the CPU.

A case is a dict: kind, name, the keyword arguments of helpers.make_params, `inputs` (name -> float64 array holding float32
representable values; int64 for class labels), `diff` (the inputs that get a gradient) and at most one of
    scale    the loss is multiplied by it before backward() (an upstream gradient other than 1),
    extra    the name of a differentiable input x: 0.25 * (w * x).sum() is added to the loss before backward(),
    permute  the name of an input that is handed over as a non-contiguous view (stored with its last two axes swapped).
Nothing is stored: every array is closed-form or drawn from a seeded numpy.random.default_rng.

`run(case, module, dtype, device)` runs the loss of `module` (oracle.loss_fns, a mutant of it, or capsyolo_amd.loss_fns: they
share names and signatures) and `compare(kind, got, ref64)` holds the result against the reference's."""
import functools

import numpy as np
import torch

from helpers import make_params, wave

LT = 1024                       # threads of the one block of every loss kernel (csrc/loss.hip): cell += LT

# the tolerances of test_losses_golden (tests/test_gpu_kernels.py): loss and avg_iou relative, gradients (rtol, atol)
TOL = {'dark': dict(loss=5e-5, avg_iou=5e-5, grad=(2e-4, 1e-5))}
for _k in ('darkcapsule', 'darkcapsule2', 'darkcapsule3', 'capsule'):
    TOL[_k] = dict(loss=2e-5, avg_iou=5e-5, grad=(1e-4, 1e-5))


def f32(a):
    """float64 array of float32-representable values."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ generators
def dense_labels(rng, B, g, C, p_obj=0.5, width=None, half=0.0):
    """[B,g,g,width or 5+C]: a cell is an object with probability p_obj (first entry 1, centre uniform in (0,1), size uniform in
    (0.02,0.4), one class column set), with probability `half` a FRACTIONAL object (first entry 0.5, the rest as for an object: the
    capsule losses use the entry as a number, dark_loss skips such a cell), and empty (all zeros) otherwise."""
    width = 5 + C if width is None else width
    y = np.zeros((B, g, g, width))
    u = rng.uniform(0.0, 1.0, (B, g, g))
    filled = u < p_obj + half
    y[..., 0] = np.where(u < p_obj, 1.0, np.where(filled, 0.5, 0.0))
    y[..., 1:3] = rng.uniform(0.0, 1.0, (B, g, g, 2)) * filled[..., None]
    y[..., 3:5] = rng.uniform(0.02, 0.4, (B, g, g, 2)) * filled[..., None]
    if width > 5:
        cls = rng.integers(0, width - 5, (B, g, g))
        y[..., 5:] = (np.arange(width - 5) == cls[..., None]) * filled[..., None]
    return f32(y)


def _dark(name, B, g, nb, C, seed, p_obj=0.5, width=None, **more):
    rng = np.random.default_rng(seed)
    y = dense_labels(rng, B, g, C, p_obj, width)
    pred = f32(rng.uniform(0.02, 0.98, (B, g, g, 5 * nb + C)))
    return dict(kind='dark', name=name, params=dict(n_boxes=nb, n_classes=C, n_grid=g, darknet_input=608 if g == 19 else 64),
                inputs=dict(y_pred=pred, y_true=y), diff=('y_pred',), **more)


def _dark_hand_built():
    """(1,2,2,0), two boxes, 64 pixels (cells of 32): the four situations no drawn input has."""
    y = np.zeros((1, 2, 2, 5))
    p = np.zeros((1, 2, 2, 10))
    # cell 0: both boxes are the same rectangle -> the two IoU are the same bits; box 0 is responsible.  Their confidences differ.
    y[0, 0, 0] = (1.0, 0.5, 0.5, 0.25, 0.25)
    p[0, 0, 0] = (0.7, 0.4, 0.6, 0.3, 0.2) + (0.2, 0.4, 0.6, 0.3, 0.2)
    # cell 1: truth [12.8,19.2]^2, box 0 = [0,3.2]^2, box 1 = [29.12,31.68]^2 -> both IoU exactly 0; box 0 is responsible, target 0
    y[0, 0, 1] = (1.0, 0.5, 0.5, 0.1, 0.1)
    p[0, 0, 1] = (0.6, 0.05, 0.05, 0.05, 0.05) + (0.3, 0.95, 0.95, 0.04, 0.04)
    # cell 2: neither an object nor empty -> nothing, and a gradient of exactly zero
    y[0, 1, 0] = (0.5, 0.3, 0.3, 0.2, 0.2)
    p[0, 1, 0] = (0.8, 0.3, 0.3, 0.2, 0.2) + (0.9, 0.5, 0.5, 0.3, 0.3)
    # cell 3: box 1 is responsible
    y[0, 1, 1] = (1.0, 0.5, 0.5, 0.3, 0.3)
    p[0, 1, 1] = (0.5, 0.2, 0.2, 0.1, 0.1) + (0.4, 0.5, 0.55, 0.28, 0.33)
    return dict(kind='dark', name='dark/hand_built', params=dict(n_boxes=2, n_classes=0, n_grid=2, darknet_input=64),
                inputs=dict(y_pred=f32(p), y_true=f32(y)), diff=('y_pred',))


def _darkcapsule(name, variant, B, g, C, seed, width=None, D=21, zero_capsule=False, **more):
    """Capsule values normal x 0.3; labels with objects, fractional objects and empty cells (dense_labels)."""
    rng = np.random.default_rng(seed)
    width = 5 + C if width is None else width
    y = dense_labels(rng, B, g, width - 5, 0.4, width, half=0.2)
    shape = {1: (B, g, g, 5), 2: (B, g, g, 5 + C), 3: (B, g, g, C, D)}[variant]
    caps = f32(0.3 * rng.standard_normal(shape))
    if zero_capsule:
        caps[0, 0, 1] = 0.0                                             # the capsule of cell 1: its length has no gradient at 0
    kind = 'darkcapsule' if variant == 1 else 'darkcapsule%d' % variant
    return dict(kind=kind, name=name, params=dict(n_classes=C, n_grid=g, recon=False), inputs=dict(caps=caps, y=y), diff=('caps',), **more)


def _capsule(name, B, C, seed, recon=False, **more):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, B)
    y[0], y[-1] = 0, C - 1                                              # class 0 and class C - 1 are there
    inputs = dict(scores=f32(rng.uniform(0.0, 1.0, (B, C))), y=y.astype(np.int64))
    diff = ('scores',)
    if recon:
        inputs['x'] = f32(wave((B, 3, 32, 32), 0.1, amp=0.9, freq=0.211))
        inputs['recon'] = f32(rng.uniform(-1.0, 1.0, (B, 3, 32, 32)))
        diff = ('scores', 'recon')
    return dict(kind='capsule', name=name, params=dict(n_classes=C, recon=recon, recon_coef=5e-4), inputs=inputs, diff=diff, **more)


def _build():
    cases = [
        _dark('dark/one_cell', 1, 1, 2, 0, seed=11, p_obj=1.0),
        _dark('dark/2x4_nb4_c3', 2, 4, 4, 3, seed=100),
        _dark('dark/3x19_nb1_c0', 3, 19, 1, 0, seed=13),
        _dark('dark/3x19_nb2_c0', 3, 19, 2, 0, seed=102),
        _dark('dark/3x19_nb3_c3', 3, 19, 3, 3, seed=100),
        _dark('dark/3x19_nb4_c43', 3, 19, 4, 43, seed=101),
        _dark_hand_built(),
        _dark('dark/all_objects', 2, 5, 2, 3, seed=100, p_obj=1.0),
        _dark('dark/no_object', 2, 3, 2, 3, seed=18, p_obj=0.0),
        _dark('dark/wide_labels', 2, 4, 2, 0, seed=19, width=48),
        _dark('dark/scaled', 2, 4, 2, 3, seed=100, scale=-1.5),
        _dark('dark/added', 2, 4, 2, 3, seed=104, extra='y_pred'),
        _dark('dark/permuted', 2, 4, 2, 3, seed=105, permute='y_pred'),
        _darkcapsule('darkcapsule/3x19_w5', 1, 3, 19, 0, seed=31),
        _darkcapsule('darkcapsule/3x19_w48', 1, 3, 19, 43, seed=32),
        _darkcapsule('darkcapsule/2x2_w5', 1, 2, 2, 0, seed=33),
        _darkcapsule('darkcapsule/2x2_w8', 1, 2, 2, 3, seed=34),
        _darkcapsule('darkcapsule/zero_capsule', 1, 2, 2, 3, seed=35, zero_capsule=True),
        _darkcapsule('darkcapsule/scaled', 1, 2, 2, 3, seed=36, scale=-1.5),
        _darkcapsule('darkcapsule/added', 1, 2, 2, 3, seed=37, extra='caps'),
        _darkcapsule('darkcapsule/permuted', 1, 2, 2, 3, seed=38, permute='y'),
        _darkcapsule('darkcapsule2/3x19_c43', 2, 3, 19, 43, seed=41),
        _darkcapsule('darkcapsule2/2x2_c3', 2, 2, 2, 3, seed=42),
        _darkcapsule('darkcapsule2/scaled', 2, 2, 2, 3, seed=43, scale=-1.5),
        _darkcapsule('darkcapsule2/added', 2, 2, 2, 3, seed=44, extra='caps'),
        _darkcapsule('darkcapsule2/permuted', 2, 2, 2, 3, seed=45, permute='caps'),
        _darkcapsule('darkcapsule3/3x19_c43_d21', 3, 3, 19, 43, seed=51),
        _darkcapsule('darkcapsule3/2x2_c3_d21', 3, 2, 2, 3, seed=52),
        _darkcapsule('darkcapsule3/2x2_c3_d9', 3, 2, 2, 3, seed=53, D=9),
        _darkcapsule('darkcapsule3/2x2_c1_d21', 3, 2, 2, 1, seed=54),
        _darkcapsule('darkcapsule3/3x19_c1_d9', 3, 3, 19, 1, seed=55, D=9),
        _darkcapsule('darkcapsule3/scaled', 3, 2, 2, 3, seed=56, scale=-1.5),
        _darkcapsule('darkcapsule3/added', 3, 2, 2, 3, seed=57, extra='caps'),
        _darkcapsule('darkcapsule3/permuted', 3, 2, 2, 3, seed=58, D=9, permute='caps'),
        _capsule('capsule/1x1', 1, 1, seed=61),
        _capsule('capsule/25x43', 25, 43, seed=62),
        _capsule('capsule/5x43_recon', 5, 43, seed=63, recon=True),
        _capsule('capsule/scaled', 5, 43, seed=64, recon=True, scale=-1.5),
        _capsule('capsule/added', 5, 43, seed=65, recon=True, extra='recon'),
        _capsule('capsule/permuted', 5, 43, seed=66, permute='scores'),
    ]
    table = dict((c['name'], c) for c in cases)
    assert len(table) == len(cases)
    return table


CASES = _build()
FN = {'dark': 'dark_loss', 'darkcapsule': 'darkcapsule_loss', 'darkcapsule2': 'darkcapsule2_loss', 'darkcapsule3': 'darkcapsule3_loss',
      'capsule': 'capsule_loss'}


def names(kind=None):
    return [n for n, c in CASES.items() if kind is None or c['kind'] == kind]


# ------------------------------------------------------------------------------------------------ running a loss
def _extra_weights(shape):
    return wave(shape, 0.9, amp=1.0, freq=0.618, dtype=np.float64)


def run(case, module, dtype=torch.float64, device='cpu', before_backward=None):
    """{'loss', 'avg_iou' (dark_loss), 'grad': {name: array}} of the case's loss as `module` computes it.  Every input goes in with
    `dtype` (class labels int64, label grids float64 as the data pipeline hands them over) on `device`."""
    p = make_params(device=str(device), **case['params'])
    labels = ('y', 'y_true')
    leaves, args = {}, {}
    for name, a in case['inputs'].items():
        t = torch.from_numpy(np.ascontiguousarray(a))
        if a.dtype != np.int64:
            t = t.to(torch.float64 if name in labels else dtype)
        if case.get('permute') == name:                                 # stored with the last two axes swapped; the view has the case's shape
            t = t.transpose(-1, -2).contiguous().to(device)
            leaf = t.requires_grad_() if name in case['diff'] else t
            view = leaf.transpose(-1, -2)
            assert not view.is_contiguous()
        else:
            leaf = t.to(device)
            if name in case['diff']:
                leaf.requires_grad_()
            view = leaf
        leaves[name], args[name] = leaf, view
    fn = getattr(module, FN[case['kind']])
    if case['kind'] == 'dark':
        out = fn(args['y_pred'], args['y_true'], p)
    elif case['kind'] == 'capsule':
        out = fn(args['scores'], args['y'], p, args.get('x'), args.get('recon'))
    else:
        out = fn(args['caps'], args['y'], p)
    loss, avg_iou = out if isinstance(out, tuple) else (out, getattr(p, 'avg_iou', None))
    total = loss
    if 'scale' in case:
        total = case['scale'] * loss
    if 'extra' in case:
        x = args[case['extra']]
        w = torch.from_numpy(_extra_weights(tuple(x.shape))).to(device=x.device, dtype=x.dtype)
        total = loss + 0.25 * (w * x).sum()
    if before_backward is not None:
        before_backward()
    total.backward()
    got = dict(loss=loss.detach().cpu().numpy(), grad={})
    if case['kind'] == 'dark':
        got['avg_iou'] = avg_iou.detach().cpu().numpy() if torch.is_tensor(avg_iou) else np.asarray(avg_iou)
    for name in case['diff']:
        g = leaves[name].grad
        g = g.transpose(-1, -2) if case.get('permute') == name else g
        got['grad'][name] = g.detach().cpu().numpy()
    return got


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 oracle's result of a case: computed once, shared, never changed (the arrays are read-only)."""
    from oracle import loss_fns as OL
    ref = run(CASES[name], OL, torch.float64)
    for a in [ref['loss']] + list(ref['grad'].values()):
        a.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------ the comparison
def _fraction(got, ref, rtol, atol):
    """Largest |got - ref| / (atol + rtol |ref|) over the whole array; NaN where the reference has NaN and nowhere else (inf there)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape:
        return float('inf')
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return float('inf')
    ok = ~nan_r
    if not ok.any():
        return 0.0
    if not np.isfinite(got[ok]).all():
        return float('inf')
    bound = atol + rtol * np.abs(ref[ok])
    err = np.abs(got[ok] - ref[ok])
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err == 0.0, 0.0, err / bound)
    return float(frac.max())


def fractions(kind, got, ref64):
    """Every compared quantity's largest error as a fraction of its tolerance: {'loss': f, 'avg_iou': f, 'grad:<name>': f}."""
    tol = TOL[kind]
    out = {'loss': _fraction(got['loss'], ref64['loss'], tol['loss'], 0.0)}
    if kind == 'dark':
        out['avg_iou'] = _fraction(got['avg_iou'], ref64['avg_iou'], tol['avg_iou'], 0.0)
    assert sorted(got['grad']) == sorted(ref64['grad'])
    for name, g in got['grad'].items():
        out['grad:' + name] = _fraction(g, ref64['grad'][name], *tol['grad'])
    return out


def compare(kind, got, ref64):
    """Assert that `got` is the reference's result within the tolerances of test_losses_golden; the whole of every gradient is
    compared, NaN included (a NaN is right exactly where the reference has one).  Returns the error fractions."""
    fr = fractions(kind, got, ref64)
    bad = dict((k, v) for k, v in fr.items() if not v <= 1.0)
    assert not bad, 'outside the tolerance (error / tolerance): %s' % bad
    return fr


def accepts(kind, got, ref64):
    try:
        compare(kind, got, ref64)
        return True
    except AssertionError:
        return False

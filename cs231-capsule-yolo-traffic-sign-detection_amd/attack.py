"""Gradients with respect to the input image, and what is built on them for the two classifiers (``capsule``, and ``cnn`` with
``"cnn_kernels": "hip"``): FGSM / PGD perturbations inside an L-infinity ball, the accuracy under them, and a saliency map.

The image gradient runs through the models' own autograd Functions (ops.py): the loss Functions, the routing / linear / max-pool
input gradients that training uses, the eval-mode BatchNorm blocks' input gradient, and at the bottom the image-gradient kernel of
the first layer (csrc/image_grad.hip).  The attack step and the saliency map are one kernel each (csrc/attack.hip).  Images are
float32 NCHW device tensors on the centred scale (u8 - 128) / 128, where 1 / 128 is one grey level; ``lo`` / ``hi`` default to the
ends of that scale.  Nothing here draws random numbers: PGD starts at the image unless the caller hands it a start.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import metrics, ops
from ._lib import HipExtensionError, call

LO, HI = -1.0, 127.0 / 128.0        # bytes 0 and 255 on the centred scale
GREY = 1.0 / 128.0                  # one grey level


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _image(x, who):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and int(x.shape[1]) == 3):
        raise HipExtensionError('%s: images must be a float32 NCHW tensor [B,3,H,W] on the GPU; there is no CPU fallback' % who)
    return x.detach().contiguous()


@contextlib.contextmanager
def _frozen(model):
    """Every parameter's requires_grad switched off inside, and put back afterwards (also on an exception): no weight gradient is
    computed, and the model's .grad fields stay what they were."""
    flags = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        yield
    finally:
        for p, was in flags:
            p.requires_grad_(was)


@contextlib.contextmanager
def _eval_mode(model):
    """The model in eval mode inside; every module's own mode is restored afterwards (also on an exception)."""
    modes = [(m, m.training) for m in model.modules()]
    try:
        model.eval()
        yield
    finally:
        for m, was in modes:
            m.training = was
        ops._bump_param_epoch()      # a switch of mode starts a new epoch of the eval-fold cache (models.HipBatchNorm2d.train)


def input_gradient(model, x, y, params, loss_fn):
    """(g, loss): g = dL/dx with the shape of x, L = loss_fn(model(x), y, params) on the model AS IT STANDS (eval or train mode is
    the caller's choice; in train mode BatchNorm runs on batch statistics and updates its running ones, as any training forward
    does).  loss is a detached 0-d device tensor.  No parameter gets a gradient."""
    xg = _image(x, 'input_gradient').requires_grad_(True)
    with _frozen(model), torch.enable_grad():
        loss = loss_fn(model(xg), y, params)
        (g,) = torch.autograd.grad(loss, xg)
    return g, loss.detach()


def attack_step(x, x0, g, alpha, eps, lo=LO, hi=HI):
    """In place on x: one signed-gradient step of size alpha, projected into the eps ball around x0 and into [lo, hi]
    (capsyolo_hip.h: cy_attack_step, where the rule is stated rounding by rounding).  Returns x."""
    for name, t in (('x', x), ('x0', x0), ('g', g)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape):
            raise HipExtensionError('attack_step: %s must be a contiguous float32 GPU tensor of the shape of x' % name)
    call('cy_attack_step', C.c_void_p(x.data_ptr()), C.c_void_p(x0.data_ptr()), C.c_void_p(g.data_ptr()), float(alpha), float(eps),
         float(lo), float(hi), x.numel(), _stream())
    return x


def pgd(model, x, y, params, loss_fn, eps, alpha, steps, start=None, lo=LO, hi=HI):
    """x_adv after `steps` signed-gradient steps of size alpha from `start` (default: x itself), each projected into the eps ball
    around x and into [lo, hi].  eps and alpha in input units (attack.GREY = 1 / 128 is one grey level).  The model runs in eval
    mode and gets its modes back; nothing crosses to the host inside the loop."""
    x0 = _image(x, 'pgd')
    xa = (x0 if start is None else _image(start, 'pgd')).clone()
    if xa.shape != x0.shape:
        raise HipExtensionError('pgd: start %s must have the shape of x %s' % (tuple(xa.shape), tuple(x0.shape)))
    if not (eps >= 0 and alpha >= 0 and int(steps) >= 0 and lo <= hi):
        raise ValueError('pgd: eps=%r alpha=%r steps=%r lo=%r hi=%r (eps, alpha, steps >= 0 and lo <= hi)' % (eps, alpha, steps, lo, hi))
    with _eval_mode(model):
        for _ in range(int(steps)):
            g, _loss = input_gradient(model, xa, y, params, loss_fn)
            attack_step(xa, x0, g, alpha, eps, lo, hi)
    return xa


def fgsm(model, x, y, params, loss_fn, eps, lo=LO, hi=HI):
    """x_adv = clip(x + eps * sign(dL/dx), lo, hi): one step of size eps (the same launches as pgd(..., alpha=eps, steps=1))."""
    return pgd(model, x, y, params, loss_fn, eps, eps, 1, None, lo, hi)


def saliency(model, x, y, params, loss_fn):
    """uint8 [B,H,W] on the device: per pixel the largest |dL/dx| over the three channels, scaled by the image's own maximum to
    0..255 (capsyolo_hip.h: cy_grad_saliency_u8).  The model as it stands, like input_gradient."""
    g, _loss = input_gradient(model, x, y, params, loss_fn)
    return grad_saliency_u8(g)


def grad_saliency_u8(g):
    """The saliency map of an image gradient g [B,3,H,W] (float32, GPU): uint8 [B,H,W]."""
    g = _image(g, 'grad_saliency_u8')
    B, _, H, W = (int(v) for v in g.shape)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=g.device)
    call('cy_grad_saliency_u8', C.c_void_p(g.data_ptr()), C.c_void_p(out.data_ptr()), B, H, W, _stream())
    return out


def _chunks(x_np, y_np, params, batch_size):
    """The batches of predict_fns.class_scores_device (same slices, same conversion), with their labels."""
    n = int(x_np.shape[0])
    bs = max(n if not batch_size else int(batch_size), 1)
    for lo in range(0, n, bs):
        xt = torch.from_numpy(np.ascontiguousarray(x_np[lo:lo + bs])).to(device=params.device, dtype=torch.float32)
        yt = torch.from_numpy(np.ascontiguousarray(y_np[lo:lo + bs])).to(device=params.device, dtype=torch.int64)
        yield xt.permute(0, 3, 1, 2).contiguous(), yt


def robust_accuracy(model, x_np, y_np, params, loss_fn, eps_list, attack='fgsm', alpha=None, steps=0, batch_size=1024):
    """{eps: accuracy} of the classifier on x_np (NHWC numpy on the centred scale) with labels y_np, every sample moved by the
    attack inside its eps ball first (eps in input units; eps == 0: the clean samples, exactly metrics.recog_acc of the clean
    scores).  attack 'fgsm', or 'pgd' with `steps` steps of size `alpha`.  The scores stay on the device, where the arg-max and the
    count are taken (metrics.recog_counts): one read per eps."""
    if attack not in ('fgsm', 'pgd'):
        raise ValueError("robust_accuracy: attack %r, expected 'fgsm' or 'pgd'" % (attack,))
    if attack == 'pgd' and not (alpha is not None and alpha > 0 and int(steps) >= 1):
        raise ValueError('robust_accuracy: pgd needs alpha > 0 and steps >= 1 (got %r, %r)' % (alpha, steps))
    x_np, y_np = np.asarray(x_np), np.asarray(y_np)
    n = int(x_np.shape[0])
    if n == 0 or len(y_np) != n:
        raise ValueError('robust_accuracy: %d samples and %d labels' % (n, len(y_np)))
    out = {}
    with _eval_mode(model):
        for eps in eps_list:
            scores, labels = [], []
            for xt, yt in _chunks(x_np, y_np, params, batch_size):
                if eps > 0:
                    xt = fgsm(model, xt, yt, params, loss_fn, eps) if attack == 'fgsm' else \
                        pgd(model, xt, yt, params, loss_fn, eps, alpha, steps)
                with torch.no_grad():
                    scores.append(model(xt).data)
                labels.append(yt)
            s = torch.cat(scores, 0) if len(scores) != 1 else scores[0]
            _counts, correct = metrics.recog_counts(torch.cat(labels), s.reshape(n, -1), int(s.numel() // n))
            out[eps] = correct / n
    return out


SUPPORTED = "--model capsule, and --model cnn with --cnn_kernels hip (params.json \"cnn_kernels\": \"hip\")"


def parse_grey_levels(text, what='--eps'):
    """'0,1,2,4,8' -> [0.0, 1.0, 2.0, 4.0, 8.0]: a comma-separated list of finite grey levels >= 0, at least one.  ValueError with
    a message otherwise."""
    vals = []
    for part in str(text).split(','):
        try:
            v = float(part)
        except ValueError:
            raise ValueError('%s %r: %r is not a number (a comma-separated list of grey levels, e.g. 0,1,2,4,8)' % (what, text, part))
        if not (np.isfinite(v) and v >= 0):
            raise ValueError('%s %r: grey levels are finite and >= 0, got %r' % (what, text, part))
        vals.append(v)
    if not vals:
        raise ValueError('%s: no grey levels given' % what)
    return vals

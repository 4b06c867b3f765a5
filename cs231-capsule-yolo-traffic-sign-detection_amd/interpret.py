"""Capsule interpretation (the reference's capsule_interpret.py) and reconstruction outside the training loss, on the fused decoder
kernel (csrc/decoder.hip, `cy_decoder_fwd`: the whole decoder forward of one capsule vector in one workgroup).

capsule_interpret.py:54-68 takes one sample, picks the 16-vector of its true class out of traffic_sign_capsules, adds each of 11
offsets to each of the 16 components in turn and writes the 176 decoded images.  Here the gather, the perturbation, the decoder and
the conversion to bytes are ONE launch for all N * 16 * len(deltas) rows.  The reference perturbs in place (`t[v] += c ... t[v] -=
c`), which lets `t` drift by rounding (measured: <= 1.8e-8); here every row is the clean `t[v] + c`.

The byte conversion is `v * 128 + 128`, rounded half to even, clamped to 0..255: what cv2.imwrite is understood to do with a float
image (cvRound + saturate_cast).  cv2 is not a dependency, so that equivalence is NOT verified.  Images are written as binary PPM
(neither cv2 nor a PNG encoder is available).  There is no CPU fallback and nothing here imports the oracle."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import call
from .ops import _f32

DELTAS = (np.arange(11) * 0.05 - 0.25).astype(np.float32)          # capsule_interpret.py:59; element 5 is exactly 0

_DECODER_KEYS = (('lin_w', 0, 'weight', (256, 16)), ('lin_b', 0, 'bias', (256,)), ('w4', 4, 'weight', (4, 16, 3, 3)),
                 ('b4', 4, 'bias', (4,)), ('w7', 7, 'weight', (8, 4, 3, 3)), ('b7', 7, 'bias', (8,)),
                 ('w10', 10, 'weight', (16, 8, 3, 3)), ('b10', 10, 'bias', (16,)), ('w12', 12, 'weight', (3, 16, 3, 3)),
                 ('b12', 12, 'bias', (3,)))


def _labels(y, n, who):
    lab = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y)
    if lab.is_floating_point() or lab.dtype == torch.bool or lab.dim() != 1 or int(lab.shape[0]) != n:
        raise ValueError('%s: labels %s %s for %d samples' % (who, lab.dtype, tuple(lab.shape), n))
    return lab.to(device='cuda', dtype=torch.int64).contiguous()


def _decode(who, model, caps, n, n_classes, labels=None, deltas=None, x=None, f32=False, u8=False, sqerr=False):
    """One `cy_decoder_fwd` launch.  caps: dense [n,16] (labels None) or [n,C,16]; returns {'f32', 'u8', 'sqerr'} (those asked for)
    with rows = n * 16 * len(deltas) (deltas given) or n leading entries."""
    dec = model.decoder
    keep = [caps, labels, deltas, x]                          # the tensors behind the raw pointers, alive until the launch is queued
    a = _lib.Decoder(caps=caps.data_ptr(), labels=None if labels is None else labels.data_ptr(),
                     deltas=None if deltas is None else deltas.data_ptr(), x=None if x is None else x.data_ptr(),
                     n=n, C=n_classes, D=16, n_delta=0 if deltas is None else int(deltas.numel()))
    for field, idx, name, shape in _DECODER_KEYS:
        p = _f32(getattr(dec[idx], name).detach(), 'decoder.%d.%s' % (idx, name))
        if tuple(p.shape) != shape:
            raise ValueError('%s: decoder.%d.%s has shape %s, not %s' % (who, idx, name, tuple(p.shape), shape))
        keep.append(p)
        setattr(a, field, p.data_ptr())
    rows = n * (16 * a.n_delta if deltas is not None else 1)
    out = {}
    if f32:
        out['f32'] = torch.empty((rows, 3, 32, 32), dtype=torch.float32, device='cuda')
        a.out_f32 = out['f32'].data_ptr()
    if u8:
        out['u8'] = torch.empty((rows, 32, 32, 3), dtype=torch.uint8, device='cuda')
        a.out_u8 = out['u8'].data_ptr()
    if sqerr:
        out['sqerr'] = torch.empty((rows,), dtype=torch.float32, device='cuda')
        a.sqerr = out['sqerr'].data_ptr()
    err = None
    if labels is not None:
        err = torch.zeros(1, dtype=torch.int32, device='cuda')
        a.err = err.data_ptr()
    call('cy_decoder_fwd', C.byref(a), torch.cuda.current_stream().cuda_stream)
    if err is not None:
        bad = int(err.item())
        if bad:
            raise ValueError('%s: %d row(s) with a label outside 0..%d' % (who, bad, n_classes - 1))
    del keep
    return out


def decode_capsules(model, t, u8=False):
    """The decoder of `model` (a CapsuleNet) on t [n,16] float32 device tensor: reconstructions float32 [n,3,32,32] (the decoder's
    NCHW), or with u8 the bytes [n,32,32,3] (see the module docstring).  n = 0: an empty tensor, no launch."""
    t = _f32(t, 'capsule vectors')
    if t.dim() != 2 or int(t.shape[1]) != 16:
        raise ValueError('decode_capsules: capsule vectors of shape %s, expected [n, 16]' % (tuple(t.shape),))
    n = int(t.shape[0])
    if n == 0:
        return torch.empty((0, 32, 32, 3), dtype=torch.uint8, device=t.device) if u8 else \
            torch.empty((0, 3, 32, 32), dtype=torch.float32, device=t.device)
    return _decode('decode_capsules', model, t, n, 1, f32=not u8, u8=u8)['u8' if u8 else 'f32']


def _nchw_device(x, who):
    """NHWC images [N,32,32,3], numpy or tensor -> float32 NCHW on the device (main.py:57-59)."""
    xt = torch.as_tensor(np.ascontiguousarray(x) if not torch.is_tensor(x) else x)
    if xt.dim() != 4 or tuple(xt.shape[1:]) != (32, 32, 3):
        raise ValueError('%s: images of shape %s, expected [N, 32, 32, 3]' % (who, tuple(xt.shape)))
    return xt.to(device='cuda', dtype=torch.float32).permute(0, 3, 1, 2).contiguous()


def reconstruct(model, x, y, params, batch_size=1024):
    """(recon float32 [N,3,32,32], sqerr float32 [N]) on the device for NHWC images x and labels y: the decoder's image of every
    sample's labelled capsule and sum((x - recon)^2) over its 3 072 elements, the per-sample term capsule_loss sums
    (loss_fns.py: recon_coef * sum).  Eval mode, no_grad, chunks of batch_size samples."""
    xt = _nchw_device(x, 'reconstruct')
    n = int(xt.shape[0])
    lab = _labels(y, n, 'reconstruct')
    if n == 0:
        raise ValueError('reconstruct: no samples')
    n_classes = int(params.n_classes)
    bs = max(int(batch_size) if batch_size else n, 1)
    model.eval()
    recon, sqerr = [], []
    with torch.no_grad():
        for lo in range(0, n, bs):
            xb, lb = xt[lo:lo + bs], lab[lo:lo + bs]
            caps = _f32(model.capsules(xb), 'capsules')
            out = _decode('reconstruct', model, caps, int(xb.shape[0]), n_classes, labels=lb, x=xb, f32=True, sqerr=True)
            recon.append(out['f32'])
            sqerr.append(out['sqerr'])
    return (torch.cat(recon), torch.cat(sqerr)) if len(recon) != 1 else (recon[0], sqerr[0])


def perturb_sweep(model, caps, y, deltas=DELTAS, u8=True):
    """capsule_interpret.py:58-68 for N samples in one launch: caps [N,C,16] float32 device tensor (CapsuleNet.capsules), y [N]
    labels (numpy or tensor).  Row (b, v, i) decodes caps[b, y[b], :] with float32(deltas[i]) added to component v.  Returns uint8
    [N,16,len(deltas),32,32,3], or with u8=False float32 [N,16,len(deltas),3,32,32].  ValueError: a label outside 0..C-1."""
    caps = _f32(caps, 'capsules')
    if caps.dim() != 3 or int(caps.shape[2]) != 16 or int(caps.shape[0]) < 1 or int(caps.shape[1]) < 1:
        raise ValueError('perturb_sweep: capsules of shape %s, expected [N, C, 16]' % (tuple(caps.shape),))
    n, n_classes = int(caps.shape[0]), int(caps.shape[1])
    lab = _labels(y, n, 'perturb_sweep')
    d = np.ascontiguousarray(np.asarray(deltas, dtype=np.float32).reshape(-1))
    if len(d) < 1:
        raise ValueError('perturb_sweep: no deltas')
    dt = torch.from_numpy(d).cuda()
    out = _decode('perturb_sweep', model, caps, n, n_classes, labels=lab, deltas=dt, f32=not u8, u8=u8)
    return out['u8'].view(n, 16, len(d), 32, 32, 3) if u8 else out['f32'].view(n, 16, len(d), 3, 32, 32)


def interpret_sample(model, x_one, y_one, params, deltas=DELTAS, u8=True):
    """capsule_interpret.py:42-68 for one NHWC sample x_one [32,32,3] with label y_one: capsules, then the sweep of the labelled
    capsule's 16 components.  Returns a dict: 'sweep' ([16,len(deltas),32,32,3] uint8 or, with u8=False, [16,len(deltas),3,32,32]
    float32; device), 'caps' [C,16], 'recon' [3,32,32] the unperturbed reconstruction, 'sqerr' (float) its squared error against
    the sample, 'label' and 'pred' (argmax of the capsule lengths)."""
    x_one = torch.as_tensor(np.ascontiguousarray(x_one) if not torch.is_tensor(x_one) else x_one)
    if x_one.dim() != 3:
        raise ValueError('interpret_sample: one sample [32, 32, 3], got shape %s' % (tuple(x_one.shape),))
    xt = _nchw_device(x_one[None], 'interpret_sample')
    lab = _labels(np.asarray([int(y_one)]), 1, 'interpret_sample')
    model.eval()
    with torch.no_grad():
        caps = _f32(model.capsules(xt), 'capsules')
        sweep = perturb_sweep(model, caps, lab, deltas, u8)
        plain = _decode('interpret_sample', model, caps, 1, int(caps.shape[1]), labels=lab, x=xt, f32=True, sqerr=True)
    return {'sweep': sweep[0], 'caps': caps[0], 'recon': plain['f32'][0], 'sqerr': float(plain['sqerr'][0].item()),
            'label': int(y_one), 'pred': int(torch.argmax((caps[0] * caps[0]).sum(dim=1)).item())}


def to_bytes(x):
    """An input image on the (v - 128) / 128 scale (numpy) -> uint8 by the rule of the kernel's byte output."""
    return np.clip(np.rint(np.asarray(x, dtype=np.float32) * np.float32(128.0) + np.float32(128.0)), 0, 255).astype(np.uint8)


def contact_sheet(sweep_u8):
    """[V,I,h,w,3] -> one image [V*h, I*w, 3]: row v, column i."""
    s = np.asarray(sweep_u8)
    v, i, h, w, c = s.shape
    return np.ascontiguousarray(s.transpose(0, 2, 1, 3, 4).reshape(v * h, i * w, c))


def write_ppm(path, bgr_u8):
    """Binary PPM (P6) of a uint8 image [h,w,3] in cv2's channel order (BGR, what cv2.imwrite would be handed): the channels are
    flipped to the RGB a PPM holds."""
    a = np.asarray(bgr_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('write_ppm: expected a uint8 array [h, w, 3], got %s %s' % (a.dtype, a.shape))
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[:, :, ::-1]).tobytes())


def read_ppm(path):
    """The inverse of write_ppm: uint8 [h,w,3] back in BGR order."""
    with open(path, 'rb') as f:
        raw = f.read()
    magic, dims, maxval, body = raw.split(b'\n', 3)
    w, h = (int(v) for v in dims.split())
    if magic != b'P6' or maxval != b'255' or len(body) != w * h * 3:
        raise ValueError('read_ppm: %s is not a binary 8-bit PPM written by write_ppm' % path)
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)[:, :, ::-1].copy()

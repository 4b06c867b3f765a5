"""numpy restatements of the three rules of include/capsyolo_hip.h that tests/test_attack_host.py and the GPU tests hold the
kernels to: the gradient with respect to the image (fp64, or int64 for the exact test; loops over the taps, no transposed
convolution), the attack step (fp32, one rounding per operation) and the saliency map."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def dz_of(dy, act=None, slope=1.0, scale=None):
    """dz = dy * (act > 0 ? 1 : slope) * scale[co] in the dtype of dy (NHWC; act and scale optional)."""
    dz = np.array(dy, copy=True)
    if act is not None:
        dz = dz * np.where(np.asarray(act) > 0, dz.dtype.type(1), dz.dtype.type(slope))
    if scale is not None:
        dz = dz * np.asarray(scale).astype(dz.dtype)[None, None, None, :]
    return dz


def image_grad(dy, w, H, W, pad, act=None, slope=1.0, scale=None, dtype=np.float64):
    """dx[B,3,H,W] from dy[B,Ho,Wo,Cout] (NHWC) and w[Cout,Cin,k,k]:
         dx[b,c,y,x] = sum_co sum_kh sum_kw dz[b, y+pad-kh, x+pad-kw, co] * w[co,c,kh,kw], terms off the map absent.
    dtype float64 (the reference) or int64 (integer inputs: the exact result).  Also returns the largest |partial sum| bound: the sum
    of |terms| per element, which bounds every partial sum of every summation order."""
    dy = np.asarray(dy).astype(dtype)
    w = np.asarray(w).astype(dtype)
    B, Ho, Wo, Cout = dy.shape
    _, Cin, k, _ = w.shape
    assert (Ho, Wo) == (H + 2 * pad - k + 1, W + 2 * pad - k + 1)
    dz = dz_of(dy, act, slope, None if scale is None else np.asarray(scale).astype(dtype))
    dx = np.zeros((B, Cin, H, W), dtype=dtype)
    mag = np.zeros((B, Cin, H, W), dtype=dtype)
    for kh in range(k):
        for kw in range(k):
            # image rows y with 0 <= y + pad - kh < Ho
            y0, y1 = max(0, kh - pad), min(H, Ho + kh - pad)
            x0, x1 = max(0, kw - pad), min(W, Wo + kw - pad)
            if y0 >= y1 or x0 >= x1:
                continue
            piece = dz[:, y0 + pad - kh:y1 + pad - kh, x0 + pad - kw:x1 + pad - kw, :]            # [B,h,w,Cout]
            dx[:, :, y0:y1, x0:x1] += np.einsum('bhwo,oc->bchw', piece, w[:, :, kh, kw])
            mag[:, :, y0:y1, x0:x1] += np.einsum('bhwo,oc->bchw', np.abs(piece), np.abs(w[:, :, kh, kw]))
    return dx, mag


def attack_step(x, x0, g, alpha, eps, lo, hi):
    """The rule of cy_attack_step in fp32, one rounding per operation:
         s = (g > 0) - (g < 0); t = x + alpha * s; t = min(max(t, x0 - eps), x0 + eps); x = min(max(t, lo), hi)."""
    x, x0, g = (np.asarray(a, dtype=F32) for a in (x, x0, g))
    alpha, eps, lo, hi = F32(alpha), F32(eps), F32(lo), F32(hi)
    with np.errstate(invalid='ignore'):
        s = (g > 0).astype(F32) - (g < 0).astype(F32)            # NaN compares false twice: 0
        t = (x + alpha * s).astype(F32)
        t = np.minimum(np.maximum(t, (x0 - eps).astype(F32)), (x0 + eps).astype(F32))
        return np.minimum(np.maximum(t, lo), hi).astype(F32)


def saliency_u8(g):
    """The rule of cy_grad_saliency_u8: m = max_c |g| (NaN -> 0, inf -> FLT_MAX), out = floor(m / max_image * 255 + 0.5) with the
    quotient, the product and the sum each rounded to fp32; an image whose maximum is 0 gives zeros.  g [B,3,H,W] -> uint8 [B,H,W]."""
    a = np.abs(np.asarray(g, dtype=F32))
    a = np.where(np.isnan(a), F32(0), np.minimum(a, FLT_MAX)).astype(F32)
    m = a.max(axis=1)
    out = np.zeros(m.shape, dtype=np.uint8)
    for b in range(m.shape[0]):
        mx = m[b].max()
        if mx > 0:
            q = ((m[b] / mx).astype(F32) * F32(255)).astype(F32)
            out[b] = np.floor((q + F32(0.5)).astype(F32)).astype(np.uint8)
    return out

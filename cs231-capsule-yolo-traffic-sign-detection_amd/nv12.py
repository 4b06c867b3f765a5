"""NV12 frames: the layout and the colour rule of include/capsyolo_hip.h on the host side.

A camera or a video decode engine delivers a full-resolution Y plane and a half-resolution plane of interleaved (U, V) pairs, 1.5
bytes per pixel, usually with a row pitch wider than the frame.  `serve.SignDetector(frame_format='nv12')` reads such frames in place:
its two crop launches convert in their tap fetch.  This module holds what the host needs around that: the coefficient rows
(`MATRICES`, `YuvMatrix`, `coef`), the description of one surface (`Layout`), the whole-image conversion on the device
(`to_rgb_device`, on `cy_nv12_to_rgb_u8`) and a host ENCODER for synthetic data and tests (`from_rgb`).
"""
import collections

import numpy as np

from ._lib import YuvCoef, call

YuvMatrix = collections.namedtuple('YuvMatrix', ['y_off', 'cy', 'cvr', 'cug', 'cvg', 'cub'])

# 2^20 fixed point.  bt601: the rounded textbook factors 1.164 / 1.596 / 0.391 / 0.813 / 2.018 of video-range BT.601; the other rows
# are round(x * 2^20) of the exact Kr / Kb formulas (video range: 255/219 and 255/224 scales; *_full: full range, no offset).
MATRICES = {
    'bt601': YuvMatrix(16, 1220542, 1673527, 409993, 852492, 2116026),
    'bt709': YuvMatrix(16, 1220945, 1879825, 223607, 558796, 2215014),
    'bt601_full': YuvMatrix(0, 1048576, 1470104, 360853, 748826, 1858077),
    'bt709_full': YuvMatrix(0, 1048576, 1651297, 196424, 490864, 1945738),
}


def coef(matrix='bt601'):
    """A validated `YuvMatrix` from a name of MATRICES or six integers (y_off, cy, cvr, cug, cvg, cub)."""
    if isinstance(matrix, str):
        if matrix not in MATRICES:
            raise ValueError('yuv matrix %r: one of %s, or six integers' % (matrix, ', '.join(sorted(MATRICES))))
        return MATRICES[matrix]
    try:
        vals = list(matrix)
    except TypeError:
        raise ValueError('yuv matrix %r: a name of MATRICES or six integers' % (matrix,))
    if len(vals) != 6 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError('yuv matrix %r: six integers (y_off, cy, cvr, cug, cvg, cub)' % (matrix,))
    m = YuvMatrix(*(int(v) for v in vals))
    if not 0 <= m.y_off <= 255:
        raise ValueError('yuv matrix %r: y_off must be in 0..255' % (m,))
    # the largest magnitude before the shift, over all bytes: it must stay inside int32
    worst = 255 * abs(m.cy) + 128 * max(abs(m.cvr), abs(m.cug) + abs(m.cvg), abs(m.cub)) + (1 << 19)
    if worst > 2 ** 31 - 1:
        raise ValueError('yuv matrix %r: a value before the shift can reach %d, outside int32' % (m, worst))
    return m


def c_coef(matrix):
    """The row as the by-value argument of the C entry points."""
    return YuvCoef(*coef(matrix))


class Layout(object):
    """One NV12 surface of H x W pixels: the Y sample of (y, x) at byte y * pitch + x, its (U, V) pair at
    uv_off + (y >> 1) * pitch + 2 * (x >> 1).  Defaults: pitch = 2 * ceil(W / 2), uv_off = H * pitch (tight).  nbytes = uv_off +
    ceil(H / 2) * pitch.  Hashable: a detector keeps one state per (frames, layout)."""

    __slots__ = ('H', 'W', 'pitch', 'uv_off')

    def __init__(self, H, W, pitch=None, uv_off=None):
        for name, v in (('H', H), ('W', W), ('pitch', pitch), ('uv_off', uv_off)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError('Layout: %s must be an integer, got %r' % (name, v))
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError('Layout: a frame of %d x %d pixels' % (H, W))
        pitch = 2 * ((W + 1) // 2) if pitch is None else int(pitch)
        if pitch < 2 * ((W + 1) // 2):
            raise ValueError('Layout: pitch %d is shorter than the %d bytes of a chroma row of a frame %d wide' % (pitch, 2 * ((W + 1) // 2), W))
        uv_off = H * pitch if uv_off is None else int(uv_off)
        if uv_off < H * pitch:
            raise ValueError('Layout: uv_off %d lies inside the Y plane of %d rows of %d bytes' % (uv_off, H, pitch))
        if uv_off + ((H + 1) // 2) * pitch > 2 ** 31 - 1:
            raise ValueError('Layout: a surface of %d bytes does not fit the int32 geometry table' % (uv_off + ((H + 1) // 2) * pitch))
        object.__setattr__(self, 'H', H)
        object.__setattr__(self, 'W', W)
        object.__setattr__(self, 'pitch', pitch)
        object.__setattr__(self, 'uv_off', uv_off)

    def __setattr__(self, name, value):
        raise AttributeError('a Layout does not change')

    @property
    def nbytes(self):
        return self.uv_off + ((self.H + 1) // 2) * self.pitch

    @property
    def geom(self):
        """The image's img_geom row."""
        return (self.H, self.W, self.pitch, self.uv_off)

    def _key(self):
        return (self.H, self.W, self.pitch, self.uv_off)

    def __eq__(self, other):
        return isinstance(other, Layout) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'Layout(H=%d, W=%d, pitch=%d, uv_off=%d)' % self._key()

    def check(self, img_off, imgs_bytes):
        """The validity rule of the header for this surface at byte img_off of a buffer of imgs_bytes."""
        if img_off < 0 or img_off + self.nbytes > imgs_bytes:
            raise ValueError('%r at byte %d does not lie inside a buffer of %d bytes' % (self, img_off, imgs_bytes))

    @staticmethod
    def of(array):
        """The tight layout of a contiguous uint8 [H + H/2, W] array with even H, W (torch tensors have the same attributes; a
        row count divisible by 3 is H + H/2 of an even H)."""
        shape = tuple(array.shape)
        if len(shape) != 2 or shape[0] < 3 or shape[0] % 3 or shape[1] < 2 or shape[1] % 2:
            raise ValueError('an NV12 frame is a uint8 array [H + H/2, W] with even H and W, got shape %s' % (shape,))
        return Layout(shape[0] // 3 * 2, shape[1])


PAD = 0x55          # what from_rgb writes into the bytes no pixel owns: neither 0 nor 128, so a kernel that reads padding shows


def _inverse(m):
    """RGB -> (Y, U, V) in float64: the inverse of the 3 x 3 matrix of the row."""
    s = float(1 << 20)
    a = np.array([[m.cy / s, 0.0, m.cvr / s], [m.cy / s, -m.cug / s, -m.cvg / s], [m.cy / s, m.cub / s, 0.0]])
    return np.linalg.inv(a)


def from_rgb(rgb, matrix='bt601', layout=None):
    """A HOST encoder, for synthetic data and tests: rgb uint8 [H, W, 3] -> uint8 [layout.nbytes] (default: the tight layout; for even
    H, W then also viewable as [H + H/2, W]).  Y per pixel, chroma the rounded mean of each 2 x 2 block's (edge blocks: of the pixels
    that exist) chroma, both from the inverse of the row's matrix in float64.  Not a counterpart whose bits are promised.  Grey input
    gives U = V = 128; the bytes no pixel owns are PAD."""
    m = coef(matrix)
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError('expected a uint8 array [H, W, 3], got %s %s' % (rgb.dtype, rgb.shape))
    H, W = rgb.shape[:2]
    lay = Layout(H, W) if layout is None else layout
    if (lay.H, lay.W) != (H, W):
        raise ValueError('%r does not describe a frame of %d x %d' % (lay, H, W))
    yuv = rgb.astype(np.float64) @ _inverse(m).T                      # [H, W, (y', u, v)] with y' = Y - y_off
    out = np.full(lay.nbytes, PAD, dtype=np.uint8)
    ys = np.clip(np.rint(yuv[..., 0] + m.y_off), 0, 255).astype(np.uint8)
    for r in range(H):
        out[r * lay.pitch:r * lay.pitch + W] = ys[r]
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    # block sums and counts with zero padding: edge blocks average what exists
    pad = np.zeros((2 * h2, 2 * w2, 2))
    pad[:H, :W] = yuv[..., 1:]
    cnt = np.zeros((2 * h2, 2 * w2))
    cnt[:H, :W] = 1.0
    mean = pad.reshape(h2, 2, w2, 2, 2).sum(axis=(1, 3)) / cnt.reshape(h2, 2, w2, 2).sum(axis=(1, 3))[..., None]
    uv = np.clip(np.rint(mean + 128.0), 0, 255).astype(np.uint8).reshape(h2, 2 * w2)
    for r in range(h2):
        out[lay.uv_off + r * lay.pitch:lay.uv_off + r * lay.pitch + 2 * w2] = uv[r]
    if layout is None and H % 2 == 0 and W % 2 == 0:
        return out.reshape(H + H // 2, W)
    return out


def to_rgb_device(buf, layouts, matrix='bt601', offsets=None):
    """NV12 surfaces in one uint8 device tensor -> a list of uint8 [H, W, 3] device tensors (views of one packed buffer), by
    `cy_nv12_to_rgb_u8` on the current stream.  layouts: one `Layout` or a list; offsets: each surface's first byte (default: one
    behind the other)."""
    import torch
    if isinstance(layouts, Layout):
        layouts = [layouts]
    layouts = list(layouts)
    if not layouts or not all(isinstance(lay, Layout) for lay in layouts):
        raise ValueError('layouts: one nv12.Layout or a list of them')
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous():
        raise ValueError('buf must be a contiguous uint8 tensor on the GPU')
    nbytes = buf.numel()
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([lay.nbytes for lay in layouts])[:-1]])
    offsets = [int(o) for o in offsets]
    if len(offsets) != len(layouts):
        raise ValueError('%d offsets for %d layouts' % (len(offsets), len(layouts)))
    for lay, o in zip(layouts, offsets):
        lay.check(o, nbytes)
    sizes = [lay.H * lay.W * 3 for lay in layouts]
    out_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    dev = buf.device
    with torch.cuda.device(dev):
        out = torch.zeros(int(sum(sizes)), dtype=torch.uint8, device=dev)
        d_off = torch.tensor(offsets, dtype=torch.int64).to(dev)
        d_geom = torch.tensor([lay.geom for lay in layouts], dtype=torch.int32).to(dev)
        d_out_off = torch.from_numpy(out_off).to(dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        call('cy_nv12_to_rgb_u8', buf.data_ptr(), d_off.data_ptr(), d_geom.data_ptr(), len(layouts), nbytes, c_coef(matrix),
             out.data_ptr(), d_out_off.data_ptr(), out.numel(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if int(err.item()):
            raise ValueError('cy_nv12_to_rgb_u8 refused %d of %d surfaces' % (int(err.item()), len(layouts)))
    return [out[o:o + s].view(lay.H, lay.W, 3) for lay, o, s in zip(layouts, out_off.tolist(), sizes)]

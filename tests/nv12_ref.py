"""The NV12 colour rule and layout of include/capsyolo_hip.h restated in numpy int64, from the text of the rule:

    Y of pixel (y, x):  buf[img_off + y * pitch + x]
    (U, V) of (y, x):   buf[img_off + uv_off + (y >> 1) * pitch + 2 * (x >> 1)] and the byte after it
    y = max(Y - y_off, 0) * cy;  u = U - 128;  v = V - 128
    R = clamp((y + cvr * v             + 2^19) >> 20, 0, 255)
    G = clamp((y - cug * u - cvg * v   + 2^19) >> 20, 0, 255)
    B = clamp((y + cub * u             + 2^19) >> 20, 0, 255)

with >> the floor shift.  Nothing here imports the package: the tables are literals of their own."""
import numpy as np

MATRICES = {
    'bt601': (16, 1220542, 1673527, 409993, 852492, 2116026),
    'bt709': (16, 1220945, 1879825, 223607, 558796, 2215014),
    'bt601_full': (0, 1048576, 1470104, 360853, 748826, 1858077),
    'bt709_full': (0, 1048576, 1651297, 196424, 490864, 1945738),
}


def _row(matrix):
    return MATRICES[matrix] if isinstance(matrix, str) else tuple(int(v) for v in matrix)


def before_clamp(Y, U, V, matrix='bt601'):
    """int64 [..., 3]: the three values behind the shift and in front of the clamp, and the largest magnitude in front of the shift."""
    y_off, cy, cvr, cug, cvg, cub = _row(matrix)
    Y, U, V = (np.asarray(a, dtype=np.int64) for a in (Y, U, V))
    y = np.maximum(Y - y_off, 0) * cy
    u, v = U - 128, V - 128
    pre = np.stack(np.broadcast_arrays(y + cvr * v + (1 << 19), y - cug * u - cvg * v + (1 << 19), y + cub * u + (1 << 19)), axis=-1)
    return pre >> 20, int(np.abs(pre).max())            # numpy's >> on a signed integer is the floor shift


def convert(Y, U, V, matrix='bt601'):
    """uint8 [..., 3] = (R, G, B)."""
    return np.clip(before_clamp(Y, U, V, matrix)[0], 0, 255).astype(np.uint8)


def tight(H, W):
    """(pitch, uv_off) of the layout without padding."""
    pitch = 2 * ((W + 1) // 2)
    return pitch, H * pitch


def nbytes(H, W, pitch=None, uv_off=None):
    pitch = tight(H, W)[0] if pitch is None else pitch
    uv_off = H * pitch if uv_off is None else uv_off
    return uv_off + ((H + 1) // 2) * pitch


def sample_index(y, x, pitch, uv_off, img_off=0):
    """(byte of Y, byte of U) of pixel (y, x); V is the byte behind U."""
    return img_off + y * pitch + x, img_off + uv_off + (y >> 1) * pitch + 2 * (x >> 1)


def planes(buf, H, W, pitch=None, uv_off=None, img_off=0):
    """(Y, U, V), each int64 [H, W]: what every pixel of the frame reads."""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    p, o = tight(H, W)
    pitch = p if pitch is None else pitch
    uv_off = H * pitch if uv_off is None else uv_off
    assert pitch >= 2 * ((W + 1) // 2) and uv_off >= H * pitch and img_off >= 0
    assert img_off + uv_off + ((H + 1) // 2) * pitch <= buf.size
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    iy, iu = sample_index(yy, xx, pitch, uv_off, img_off)
    return buf[iy].astype(np.int64), buf[iu].astype(np.int64), buf[iu + 1].astype(np.int64)


def to_rgb(buf, H=None, W=None, pitch=None, uv_off=None, matrix='bt601', img_off=0):
    """uint8 [H, W, 3] of one NV12 image.  Without H, W: buf is the tight [H + H/2, W] array with even H, W."""
    if H is None:
        buf = np.asarray(buf)
        assert buf.ndim == 2 and buf.shape[0] % 3 == 0 and buf.shape[1] % 2 == 0
        H, W = buf.shape[0] // 3 * 2, buf.shape[1]
    return convert(*planes(buf, H, W, pitch, uv_off, img_off), matrix=matrix)


def random_frame(rng, H, W, pitch=None, uv_off=None, pad=0xEE):
    """A buffer of nbytes(...) bytes with random samples where the rule reads and `pad` everywhere else."""
    p, o = tight(H, W)
    pitch = p if pitch is None else pitch
    uv_off = H * pitch if uv_off is None else uv_off
    buf = np.full(nbytes(H, W, pitch, uv_off), pad, dtype=np.uint8)
    for r in range(H):
        buf[r * pitch:r * pitch + W] = rng.integers(0, 256, W, dtype=np.uint8)
    w2 = 2 * ((W + 1) // 2)
    for r in range((H + 1) // 2):
        buf[uv_off + r * pitch:uv_off + r * pitch + w2] = rng.integers(0, 256, w2, dtype=np.uint8)
    return buf

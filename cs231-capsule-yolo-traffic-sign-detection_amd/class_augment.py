"""The classifiers' augmentation (the reference's utils.py:126-143, `utils.augmentation`: a shift of up to `max_shift` pixels with zero
fill and a lightness increase of up to `max_lightness_increase` on the V channel in HSV) from a data set that is resident on the
device, through ONE kernel per batch, `cy_gather_jitter_u8` (csrc/augment.hip).  DESIGN section 6i.

The set is uploaded once as bytes; a batch is an array of sample numbers.  Per epoch the host draws two tables indexed by sample
number (jitter_tables: vectorised, from `np.random.default_rng([seed, 23, epoch])`) and uploads them together with the sample
numbers of all the epoch's batches; per batch the kernel gathers, shifts, brightens, centres and permutes NHWC -> NCHW.  A sample's
jitter depends on (seed, epoch, sample number) only: not on the batch it travels in, nor on the number of ranks.

The reference's function is dead code (commented out at main.py:56) with three bugs, none of them reproduced: it returns the HSV
result of the UNSHIFTED x (the shift is thrown away), it returns values on the 0..1 scale instead of the centred one, and it draws
one shift and one lightness per batch.  Its lightness arithmetic is pinned by tests/golden/classaug.npz.  There is no CPU fallback."""
import numpy as np
import torch

from ._lib import HipExtensionError, call

RNG_STREAM = 23                 # augment.RNG_STREAM is 17: the two augmentations never share a stream


def jitter_tables(n_set, seed, epoch, max_shift=4, max_light=0.05):
    """(shift int32 [n_set, 2] = (dy, dx) uniform on the integers -max_shift .. max_shift, light float32 [n_set] uniform on
    [0, max_light)) of one epoch, indexed by sample number.  One generator and two vectorised draws for the whole set (a generator
    per sample costs more host time per step than CapsuleNet's step has)."""
    n_set, max_shift, max_light = int(n_set), int(max_shift), float(max_light)
    if n_set < 0 or max_shift < 0 or not 0 <= max_light < np.inf:
        raise ValueError('jitter_tables: n_set %d, max_shift %d, max_light %r' % (n_set, max_shift, max_light))
    rng = np.random.default_rng([int(seed), RNG_STREAM, int(epoch)])
    shift = rng.integers(-max_shift, max_shift + 1, size=(n_set, 2)).astype(np.int32)
    light = (rng.random(n_set, dtype=np.float32) * np.float32(max_light)).astype(np.float32)
    if max_light > 0:           # the float32 product may round up to max_light itself: keep the interval half-open
        light = np.minimum(light, np.nextafter(np.float32(max_light), np.float32(0)))
    return shift, light


class ClassAugmentFeeder(object):
    """One epoch of jittered batches.  Iterates (x float32 NCHW centred, y int64) on the device like input_pipeline.DeviceFeeder,
    over `batches`, a list of arrays of sample numbers into the resident `set_u8` [n, H, W, 3] / `labels` [n] (device tensors).
    The two tables and the concatenated sample numbers travel in one upload when the feeder is made; every batch is then one
    launch on the current stream with pointer offsets into them: no per-step copy, no host synchronisation.  The kernel's error
    word is read once, when the iteration ends.  max_shift = 0 / max_light = 0 pass no table (no shift / no lightness)."""

    def __init__(self, set_u8, labels, batches, seed=0, epoch=0, max_shift=4, max_light=0.05):
        if not torch.cuda.is_available():
            raise HipExtensionError('ClassAugmentFeeder needs a GPU: the product path has no CPU fallback')
        if set_u8.dtype != torch.uint8 or set_u8.dim() != 4 or set_u8.shape[3] != 3 or not set_u8.is_cuda or not set_u8.is_contiguous():
            raise ValueError('ClassAugmentFeeder: the set is a contiguous uint8 [n, H, W, 3] tensor on the device')
        n = int(set_u8.shape[0])
        if labels.dtype != torch.int64 or tuple(labels.shape) != (n,) or labels.device != set_u8.device:
            raise ValueError('ClassAugmentFeeder: the labels are an int64 [%d] tensor beside the set' % n)
        self.set_u8, self.labels, self.n_set = set_u8, labels, n
        self.batches = [np.asarray(b, dtype=np.int64).reshape(-1) for b in batches]
        idx = np.concatenate(self.batches) if self.batches else np.zeros(0, np.int64)
        bad = idx[(idx < 0) | (idx >= n)]
        if len(bad):
            raise ValueError('ClassAugmentFeeder: sample number %d is outside the set of %d' % (int(bad[0]), n))
        self.shift, self.light = jitter_tables(n, seed, epoch, max_shift, max_light)
        # one upload: [shift 2n | light n (its bits) | sample numbers | error word]
        words = np.concatenate([self.shift.reshape(-1), self.light.view(np.int32), idx.astype(np.int32), np.zeros(1, np.int32)])
        self._words = torch.from_numpy(words).to(set_u8.device)
        base = self._words.data_ptr()
        self._p_shift = base if max_shift else None
        self._p_light = base + 8 * n if max_light else None
        self._p_index, self._p_err = base + 12 * n, base + 4 * (len(words) - 1)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        dev = self.set_u8.device
        _, H, W, _ = self.set_u8.shape
        done = 0
        for idx in self.batches:
            B = len(idx)
            x = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
            y = torch.empty((B,), dtype=torch.int64, device=dev)
            call('cy_gather_jitter_u8', self.set_u8.data_ptr(), self.labels.data_ptr(), self.n_set, H, W, self._p_shift, self._p_light,
                 self._p_index + 4 * done, B, x.data_ptr(), y.data_ptr(), self._p_err, torch.cuda.current_stream(dev).cuda_stream)
            done += B
            yield x, y
        bad = int(self._words[-1].item())
        if bad:
            raise HipExtensionError('cy_gather_jitter_u8: %d sample number(s) outside the set of %d; they are zero-filled'
                                    % (bad, self.n_set))


class ClassAugmentSource(object):
    """What `main.py --class_augment` keeps between the epochs: the training set as bytes and its labels on the device (uploaded
    once) and the epoch count.  feeder(batches) is the ClassAugmentFeeder of the next epoch."""

    def __init__(self, x_u8, y, seed, max_shift=4, max_light=0.05, device='cuda'):
        if not torch.cuda.is_available():
            raise HipExtensionError('ClassAugmentSource needs a GPU: the product path has no CPU fallback')
        x_u8, y = np.asarray(x_u8), np.asarray(y)
        if x_u8.dtype != np.uint8 or x_u8.ndim != 4 or x_u8.shape[3] != 3 or len(x_u8) == 0:
            raise ValueError('ClassAugmentSource: the set is a non-empty uint8 [n, H, W, 3] array (input_pipeline.quantize_if_exact)')
        if y.shape != (len(x_u8),) or not np.issubdtype(y.dtype, np.integer):
            raise ValueError('ClassAugmentSource: %d images and labels of shape %s, dtype %s' % (len(x_u8), y.shape, y.dtype))
        jitter_tables(0, seed, 0, max_shift, max_light)               # the ranges are checked here, not in the first epoch
        self.set_u8 = torch.from_numpy(np.ascontiguousarray(x_u8)).to(device)
        self.labels = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int64)).to(device)
        self.seed, self.max_shift, self.max_light, self.epoch = int(seed), int(max_shift), float(max_light), 0

    def feeder(self, batches):
        f = ClassAugmentFeeder(self.set_u8, self.labels, batches, self.seed, self.epoch, self.max_shift, self.max_light)
        self.epoch += 1
        return f

"""The cases of the streaming-kernel tests: one table, shared by tests/test_stream_cases_host.py (which checks on the CPU that every
case keeps its conditions, that the reference alone passes and that wrong kernels are caught) and tests/test_gpu_streaming.py (which
runs csrc/bn.hip, csrc/misc.hip and cy_channel_sum on them).

A case is a dict: kind, name, the intended launch `path` where a launcher chooses between kernels, and its inputs (float64 arrays
holding float32-representable values, float64 for what the C-ABI takes as double, int64 for labels and counters).  Nothing is stored:
every array is closed-form or drawn from a seeded numpy.random.default_rng.  Cases are built on demand (`case(name)`); the few large
ones are not kept.

`run(case, impl)` evaluates a case with `Ref()` (numpy float64, written from the definitions of nn.BatchNorm2d, nn.LeakyReLU,
nn.MaxPool2d, nn.Upsample, sigmoid / softmax, tanh and gather), `Ref(np.float32)` (the same formulas in float32 on the CPU, with
double kept where the C-ABI has double), a mutant `Ref(np.float32, mutant=...)` or `Kernels()` (the thin adapter over
capsyolo_amd._lib.call and capsyolo_amd.ops).  `compare(case, got)` holds a result against the float64 reference:
    exact   bit equality (copies, permutes, pooling, upsampling, gather; every output of a case marked exact)
    sum     |got - ref| <= 1e-6 of the terms' abs-sum (the double sums of cy_bn_bwd_reduce: the contract used all over the suite)
    rule    the rule of tests/test_gpu_linear.py: the largest error may be 20 x the largest error of the float32 CPU evaluation, both
            measured against the magnitude of the terms (|z scale| + |shift|, not the result), with a floor of 1e-6 of it; where the
            magnitude is 0 the value must be the reference's."""
import functools

import numpy as np

MARGIN = 1e-3                   # every LeakyReLU argument is at least this far from 0, every pooling window's best from its second
COPIES = 16                     # CY_STATS_COPIES: the striped copies of the convolution epilogues' statistics
STREAM_CAP, MISC_CAP = 65536, 8192      # largest grids of stream_grid (csrc/bn.hip) and grid_for (csrc/misc.hip), blocks of 256


def f32(a):
    """float64 array of float32-representable values."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ launch arithmetic, restated
def ceil_div(a, b):
    return -(-a // b)


def stream_grid(items):
    return max(1, min(STREAM_CAP, ceil_div(items, 1024)))


def misc_grid(n):
    return max(1, min(MISC_CAP, ceil_div(n, 256)))


def affine_path(P, N, affine, offset):
    """The kernel cy_affine_act launches."""
    v4 = N % 4 == 0 and not offset
    hoist = v4 and N <= 1024 and 1024 % N == 0
    nt = P * N * 4 > (128 << 20)
    if hoist and affine:
        return 'hoist_affine_nt' if nt else 'hoist_affine'
    if hoist:
        return 'hoist_plain'
    if v4:
        return 'vector_affine' if affine else 'vector_plain'
    return 'scalar'


def apply_path(N):
    return 'hoist' if N <= 1024 and 1024 % N == 0 else 'generic'


def reduce_plan(P, N):
    """cy_bn_bwd_reduce: (rpar, rows_per_block, blocks); None where the launcher refuses N."""
    if N <= 0 or N % 4 or (N // 4) & (N // 4 - 1) or N // 4 > 256:
        return None
    cw = min(N, 64)
    nsl = N // cw
    rpar = 256 // (cw // 4)
    rpb = max(ceil_div(P, ceil_div(2048, nsl)), 4 * rpar)
    rpb = ceil_div(rpb, rpar) * rpar
    return rpar, rpb, ceil_div(P, rpb) * nsl


def unrolled_and_tail(n, stride, unroll):
    """{(passes of the unrolled body, passes of the tail loop)} over the threads of a grid-stride loop of `stride` threads that takes
    `unroll` items a pass while `i + (unroll - 1) stride < n` and single items after that."""
    found = set()
    for i in {0, (n - 1) % stride, n % stride, min(stride - 1, n - 1)}:   # the first thread, those around the last item, the last thread
        u = 0
        while i + (unroll - 1) * stride < n:
            i += unroll * stride
            u += 1
        t = 0
        while i < n:
            i += stride
            t += 1
        found.add((u, t))
    return found


# ------------------------------------------------------------------------------------------------ generators
def _rng(seed):
    return np.random.default_rng(seed)


def _scale_shift(rng, N):
    """Per-channel scale (both signs, channel 0 negative) and shift, away from zero."""
    sign = np.where(rng.random(N) < 0.4, -1.0, 1.0)
    sign[0] = -1.0
    if N > 1:
        sign[1] = 1.0
    scale = f32(sign * rng.uniform(0.5, 1.5, N))
    shift = f32(np.where(rng.random(N) < 0.5, -1.0, 1.0) * rng.uniform(0.05, 0.5, N))
    return scale, shift


def _push(z, scale=None, shift=None):
    """z with every offender |z scale + shift| < MARGIN moved to where the argument is +-4 MARGIN (draw, then push)."""
    if scale is None:
        bad = np.abs(z) < MARGIN
        return f32(np.where(bad, np.where(z < 0, -4 * MARGIN, 4 * MARGIN), z))
    y = z * scale + shift
    bad = np.abs(y) < MARGIN
    target = np.where(y < 0, -4 * MARGIN, 4 * MARGIN)
    return f32(np.where(bad, (target - shift) / scale, z))


def _mean_invstd(rng, N):
    return f32(0.3 * rng.standard_normal(N)), f32(rng.uniform(0.5, 2.0, N))


def _finalize(name, N, count, seed, momentum=0.1, running=True, clamp=False):
    rng = _rng(seed)
    x = f32(rng.standard_normal((count, N)) * rng.uniform(0.5, 2.0, N) + rng.uniform(-2.0, 2.0, N))
    if clamp:
        x[:, 1] = 2.0 ** 20                                             # a constant channel
    owner = rng.choice(COPIES, size=count, p=np.array([6, 0, 3, 1, 0, 0, 2, 1, 0, 4, 1, 0, 0, 1, 1, 0]) / 20.0)
    stats = np.zeros((COPIES, N, 2))
    for cp in range(COPIES):                                            # uneven: a copy holds the rows it owns, some own none
        rows = x[owner == cp]
        stats[cp, :, 0], stats[cp, :, 1] = rows.sum(0), (rows * rows).sum(0)
    if clamp:                                                           # ... whose sum of squares lost its last bit on the way
        stats[:, 1, :] = 0.0
        stats[0, 1, 0] = count * 2.0 ** 20
        stats[0, 1, 1] = np.nextafter(count * 2.0 ** 40, 0.0)
    gamma = f32(rng.uniform(0.5, 1.5, N))
    if N >= 3:
        gamma[0], gamma[2] = 0.0, -gamma[2]
    else:
        gamma[0] = -gamma[0]
    c = dict(kind='bn_finalize', name=name, N=N, count=count, x=x, stats=stats, gamma=gamma, beta=f32(0.2 * rng.standard_normal(N)),
             momentum=momentum, eps=1e-5, nbt=41, running_mean=None, running_var=None)
    if running:
        c['running_mean'], c['running_var'] = f32(0.1 * rng.standard_normal(N)), f32(rng.uniform(0.5, 1.5, N))
    return c


def _bn_eval(name, N, seed):
    rng = _rng(seed)
    gamma = f32(rng.uniform(0.5, 1.5, N))
    gamma[-1] = -gamma[-1]
    return dict(kind='bn_eval', name=name, N=N, gamma=gamma, beta=f32(0.2 * rng.standard_normal(N)),
                running_mean=f32(0.3 * rng.standard_normal(N)), running_var=f32(rng.uniform(0.2, 2.0, N)), eps=1e-5)


def _bn_fold(name, Cout, per_out, seed, bias=True):
    rng = _rng(seed)
    c = _bn_eval(name, Cout, seed + 1)
    c.update(kind='bn_fold', Cout=Cout, per_out=per_out, W=f32(0.2 * rng.standard_normal((Cout, per_out))),
             bias=f32(0.1 * rng.standard_normal(Cout)) if bias else None)
    return c


def _affine(name, P, N, seed, path, affine=True, slope=0.1, offset=False):
    rng = _rng(seed)
    scale, shift = _scale_shift(rng, N) if affine else (None, None)
    z = f32(rng.standard_normal((P, N)))
    return dict(kind='affine_act', name=name, P=P, N=N, z=_push(z, scale, shift), scale=scale, shift=shift, slope=slope, offset=offset,
                path=path)


def _bwd(kind, name, P, N, seed, slope=0.1, **more):
    rng = _rng(seed)
    scale, shift = _scale_shift(rng, N)
    mean, invstd = _mean_invstd(rng, N)
    z = _push(f32(rng.standard_normal((P, N))), scale, shift)
    c = dict(kind=kind, name=name, P=P, N=N, z=z, da=f32(rng.standard_normal((P, N))), scale=scale, shift=shift, mean=mean, invstd=invstd,
             slope=slope)
    if kind == 'bn_bwd_apply':
        c['red'] = rng.standard_normal((N, 2)) * np.sqrt(P) * 3.0      # double sums of the size such P terms add up to
        c['param_grads'] = True
    c.update(more)
    return c


def _apply_dyadic(name, P, N, seed):
    """Every intermediate exact: powers of two for scale and invstd, halves and integers for shift and mean, small integers for z,
    eighths for the gradient and for the two means (P a power of two).  The scales are 1, 2 or 4, so the argument is an integer and a half."""
    rng = _rng(seed)
    assert P & (P - 1) == 0
    pow2 = lambda lo: f32(2.0 ** rng.integers(lo, 3, N) * np.where(rng.random(N) < 0.5, -1.0, 1.0))
    return dict(kind='bn_bwd_apply', name=name, P=P, N=N, z=f32(rng.integers(-8, 9, (P, N))), da=f32(rng.integers(-16, 17, (P, N)) / 8.0),
                scale=pow2(0), shift=f32(rng.integers(-2, 2, N) + 0.5), mean=f32(rng.integers(-1, 2, N)), invstd=np.abs(pow2(-2)),
                slope=0.125, red=rng.integers(-16, 17, (N, 2)) / 8.0 * P, param_grads=True, exact=True, path='hoist')


def _red_fold(name, N, copies, scale, seed, outs=(True, True, True), inplace=False):
    rng = _rng(seed)
    return dict(kind='bn_red_fold', name=name, N=N, copies=copies, scale=scale, red_copies=rng.standard_normal((copies, N, 2)) * 50.0,
                outs=outs, inplace=inplace)


def _act_bwd(name, n, slope, seed):
    rng = _rng(seed)
    z = _push(f32(rng.standard_normal(n)))
    zeros = np.array([0, 1, 255, 256, n // 2, n - 1])                   # hand-placed exact zeros, +0 and -0: `z > 0` is false
    z[zeros] = 0.0
    z[zeros[1::2]] = -0.0
    return dict(kind='act_bwd', name=name, n=n, z=z, da=f32(rng.standard_normal(n)), slope=slope, zeros=zeros)


def _channel_sum(name, P, N, seed, integers=True):
    rng = _rng(seed)
    dz = f32(rng.integers(-3, 4, (P, N))) if integers else f32(rng.standard_normal((P, N)))
    return dict(kind='channel_sum', name=name, P=P, N=N, dz=dz, exact=integers)


def windows(x):
    """[4, B, Ho, Wo, C]: the four positions (row-major) of every 2 x 2 window of an NHWC map; an odd last row / column is ignored."""
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    return np.stack([x[:, dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)])


def _pool(name, B, H, W, C, seed, offset=False):
    rng = _rng(seed)
    x = rng.integers(-2 ** 15, 2 ** 15, (B, H, W, C)).astype(np.float64) / 256.0
    Ho, Wo = H // 2, W // 2
    if Ho and Wo:
        w = windows(x)
        top = np.sort(w, axis=0)
        bad = top[3] - top[2] < MARGIN
        first = w.argmax(axis=0)
        for k, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):   # push: the first maximum of an offending window goes up by 1
            x[:, dy:2 * Ho:2, dx:2 * Wo:2] += np.where(bad & (first == k), 1.0, 0.0)
    return dict(kind='maxpool', name=name, x=f32(x), g=f32(rng.integers(-64, 65, (B, Ho, Wo, C)) / 8.0), offset=offset,
                path='vector' if C % 4 == 0 and not offset else 'scalar', ties=0)


# the hand-built windows, positions 0 1 / 2 3: ties of equal bits at 0/1, 1/2, 2/3 and all four, -0.0 against 0.0 both ways, all negative
TIE_WINDOWS = [((2.5, 2.5, 1.0, -1.0), 0), ((0.5, 3.0, 3.0, 1.0), 1), ((-1.0, 0.25, 7.0, 7.0), 2), ((0.75, 0.75, 0.75, 0.75), 0),
               ((-0.0, 0.0, -1.0, -2.0), 0), ((0.0, -0.0, -1.0, -2.0), 0), ((-3.0, -1.0, -2.0, -4.0), 1)]


def _pool_ties(name, C):
    x = np.zeros((1, 2, 2 * len(TIE_WINDOWS), C))
    for i, (v, _) in enumerate(TIE_WINDOWS):
        x[0, 0, 2 * i], x[0, 0, 2 * i + 1], x[0, 1, 2 * i], x[0, 1, 2 * i + 1] = v
    g = f32(np.arange(1, len(TIE_WINDOWS) * C + 1).reshape(1, 1, len(TIE_WINDOWS), C) / 8.0)
    return dict(kind='maxpool', name=name, x=x, g=g, offset=False, path='vector' if C % 4 == 0 else 'scalar', ties=6)


def _upsample(name, B, H, W, C, f, seed):
    rng = _rng(seed)
    return dict(kind='upsample', name=name, f=f, x=f32(rng.standard_normal((B, H, W, C))),
                g=f32(rng.integers(-64, 65, (B, H * f, W * f, C)) / 8.0))   # eighths: the f^2 terms add up exactly in any order


def _tanh(name, seed):
    rng = _rng(seed)
    special = [0.0, -0.0, 1e-8, -1e-8, 12.0, -12.0, 9.5, -9.5, 20.0, -40.0, 0.5, -0.5]
    x = f32(np.concatenate([special, np.linspace(-12.0, 12.0, 601), rng.uniform(-3.0, 3.0, 400)]))
    return dict(kind='tanh', name=name, x=x, g=f32(rng.standard_normal(x.size)))


def _head(name, cells, split, C, seed, big=None):
    rng = _rng(seed)
    x = f32(2.0 * rng.standard_normal((cells, split + C)))
    if big is not None:                                                 # logits of +-big in the first cells, in every pattern that matters
        x[0, :] = big
        x[1, :] = -big
        x[2, ::2], x[2, 1::2] = big, -big
        x[3, :] = -big
        x[3, -1] = big
    return dict(kind='yolo_head', name=name, cells=cells, split=split, C=C, x=x, g=f32(rng.standard_normal((cells, split + C))))


def _permute(name, op, shape, seed, n_caps=None):
    rng = _rng(seed)
    x = f32(rng.standard_normal(shape))
    c = dict(kind='permute', name=name, op=op, x=x, n_caps=n_caps)
    c['g'] = f32(rng.standard_normal(Ref().permute(dict(c, g=None))['y'].shape))
    return c


def _pick(name, B, C, D, seed):
    rng = _rng(seed)
    y = rng.integers(0, C, B)
    y[0], y[-1] = 0, C - 1
    return dict(kind='pick', name=name, caps=f32(rng.standard_normal((B, C, D))), y=y.astype(np.int64), g=f32(rng.standard_normal((B, D))))


def _reduce_cases():
    out = {}
    slopes = [0.1, 1.0, 0.0]
    k = 0
    for N in (4, 8, 32, 64, 128, 1024):
        rpar = 256 // (min(N, 64) // 4)
        for P in (1, rpar - 1, 4 * rpar, 4 * rpar + 1):
            nm = 'bn_bwd_reduce/n%d_p%d' % (N, P)
            out[nm] = functools.partial(_bwd, 'bn_bwd_reduce', nm, P, N, 300 + k, slope=slopes[k % 3])
            k += 1
    nm = 'bn_bwd_reduce/n64_two_unrolled_and_tail'
    out[nm] = functools.partial(_bwd, 'bn_bwd_reduce', nm, 2048 * 144 + 77, 64, 399, slope=0.1)
    return out


REFUSED_REDUCE_N = (12, 40, 2048)      # cy_bn_bwd_reduce takes N = 4 * 2^k <= 1024 and must refuse these with a HipExtensionError
BIG = {'affine_act/hoist_affine_nt_over_128mib', 'bn_bwd_reduce/n64_two_unrolled_and_tail', 'maxpool/vector_grid_loops',
       'maxpool/scalar_grid_loops', 'upsample/over_the_grid_cap', 'permute/nchw_to_nhwc_over_the_grid_cap'}

_P = functools.partial
FACTORY = {
    'bn_finalize/n1': _P(_finalize, 'bn_finalize/n1', 1, 7, 201),
    'bn_finalize/n3_count1': _P(_finalize, 'bn_finalize/n3_count1', 3, 1, 202),
    'bn_finalize/n3_clamp': _P(_finalize, 'bn_finalize/n3_clamp', 3, 8, 203, clamp=True),
    'bn_finalize/n256_momentum1': _P(_finalize, 'bn_finalize/n256_momentum1', 256, 37, 204, momentum=1.0),
    'bn_finalize/n257': _P(_finalize, 'bn_finalize/n257', 257, 50, 205),
    'bn_finalize/n1024_no_running': _P(_finalize, 'bn_finalize/n1024_no_running', 1024, 19, 206, running=False),
    'bn_eval/n1': _P(_bn_eval, 'bn_eval/n1', 1, 211),
    'bn_eval/n300': _P(_bn_eval, 'bn_eval/n300', 300, 212),
    'bn_fold/per_out1': _P(_bn_fold, 'bn_fold/per_out1', 7, 1, 221),
    'bn_fold/3x3_cin3': _P(_bn_fold, 'bn_fold/3x3_cin3', 5, 27, 222),
    'bn_fold/4x4_cin3_no_bias': _P(_bn_fold, 'bn_fold/4x4_cin3_no_bias', 11, 48, 223, bias=False),
    'bn_fold/3x3_cin32': _P(_bn_fold, 'bn_fold/3x3_cin32', 3, 288, 224),
    'affine_act/hoist_affine_n4': _P(_affine, 'affine_act/hoist_affine_n4', 2500, 4, 231, 'hoist_affine'),
    'affine_act/hoist_affine_n64_slope0': _P(_affine, 'affine_act/hoist_affine_n64_slope0', 157, 64, 232, 'hoist_affine', slope=0.0),
    'affine_act/hoist_affine_n1024': _P(_affine, 'affine_act/hoist_affine_n1024', 10, 1024, 233, 'hoist_affine', slope=1.0),
    'affine_act/hoist_plain_n64_relu': _P(_affine, 'affine_act/hoist_plain_n64_relu', 157, 64, 234, 'hoist_plain', affine=False, slope=0.0),
    'affine_act/hoist_affine_nt_over_128mib': _P(_affine, 'affine_act/hoist_affine_nt_over_128mib', 524289, 64, 235, 'hoist_affine_nt'),
    'affine_act/vector_affine_n40': _P(_affine, 'affine_act/vector_affine_n40', 251, 40, 236, 'vector_affine'),
    'affine_act/vector_affine_n12': _P(_affine, 'affine_act/vector_affine_n12', 837, 12, 237, 'vector_affine', slope=0.0),
    'affine_act/vector_affine_n2048': _P(_affine, 'affine_act/vector_affine_n2048', 5, 2048, 238, 'vector_affine'),
    'affine_act/vector_plain_n40': _P(_affine, 'affine_act/vector_plain_n40', 251, 40, 239, 'vector_plain', affine=False),
    'affine_act/scalar_n10': _P(_affine, 'affine_act/scalar_n10', 301, 10, 240, 'scalar'),
    'affine_act/scalar_n3_plain_slope1': _P(_affine, 'affine_act/scalar_n3_plain_slope1', 1001, 3, 241, 'scalar', affine=False, slope=1.0),
    'affine_act/scalar_n64_offset_view': _P(_affine, 'affine_act/scalar_n64_offset_view', 157, 64, 242, 'scalar', offset=True),
    'bn_bwd_apply/hoist_n4': _P(_bwd, 'bn_bwd_apply', 'bn_bwd_apply/hoist_n4', 2500, 4, 251, path='hoist'),
    'bn_bwd_apply/hoist_n256_no_param_grads': _P(_bwd, 'bn_bwd_apply', 'bn_bwd_apply/hoist_n256_no_param_grads', 39, 256, 252, slope=0.0,
                                                 path='hoist', param_grads=False),
    'bn_bwd_apply/hoist_n1024': _P(_bwd, 'bn_bwd_apply', 'bn_bwd_apply/hoist_n1024', 10, 1024, 253, slope=1.0, path='hoist'),
    'bn_bwd_apply/generic_n12': _P(_bwd, 'bn_bwd_apply', 'bn_bwd_apply/generic_n12', 837, 12, 254, path='generic'),
    'bn_bwd_apply/generic_n40_no_param_grads': _P(_bwd, 'bn_bwd_apply', 'bn_bwd_apply/generic_n40_no_param_grads', 251, 40, 255,
                                                  path='generic', param_grads=False),
    'bn_bwd_apply/generic_n2048': _P(_bwd, 'bn_bwd_apply', 'bn_bwd_apply/generic_n2048', 5, 2048, 256, path='generic'),
    'bn_bwd_apply/dyadic_exact': _P(_apply_dyadic, 'bn_bwd_apply/dyadic_exact', 32, 256, 257),
    'bn_red_fold/one_copy': _P(_red_fold, 'bn_red_fold/one_copy', 257, 1, 1.0, 261),
    'bn_red_fold/16_copies': _P(_red_fold, 'bn_red_fold/16_copies', 257, COPIES, 1.0, 262),
    'bn_red_fold/in_place_over_world': _P(_red_fold, 'bn_red_fold/in_place_over_world', 64, 1, 1.0 / 3, 263, outs=(True, False, False),
                                          inplace=True),
    'bn_red_fold/no_red_out': _P(_red_fold, 'bn_red_fold/no_red_out', 5, COPIES, 0.5, 264, outs=(False, True, True)),
    'bn_red_fold/no_dgamma': _P(_red_fold, 'bn_red_fold/no_dgamma', 5, COPIES, 0.5, 265, outs=(True, False, True)),
    'bn_red_fold/no_dbeta': _P(_red_fold, 'bn_red_fold/no_dbeta', 300, COPIES, 1.0 / 8, 266, outs=(True, True, False)),
    'act_bwd/n1000': _P(_act_bwd, 'act_bwd/n1000', 1000, 0.1, 271),
    'act_bwd/n1000_relu': _P(_act_bwd, 'act_bwd/n1000_relu', 1000, 0.0, 272),
    'channel_sum/p1_n1': _P(_channel_sum, 'channel_sum/p1_n1', 1, 1, 281),
    'channel_sum/p63_n10': _P(_channel_sum, 'channel_sum/p63_n10', 63, 10, 282),
    'channel_sum/p64_n64': _P(_channel_sum, 'channel_sum/p64_n64', 64, 64, 283),
    'channel_sum/p65_n65': _P(_channel_sum, 'channel_sum/p65_n65', 65, 65, 284),
    'channel_sum/p5000_n200': _P(_channel_sum, 'channel_sum/p5000_n200', 5000, 200, 285),
    'channel_sum/p5000_n1': _P(_channel_sum, 'channel_sum/p5000_n1', 5000, 1, 286),
    'channel_sum/p1_n200': _P(_channel_sum, 'channel_sum/p1_n200', 1, 200, 287),
    'channel_sum/normal_p5000_n64': _P(_channel_sum, 'channel_sum/normal_p5000_n64', 5000, 64, 288, integers=False),
    'maxpool/2x2_c3': _P(_pool, 'maxpool/2x2_c3', 2, 2, 2, 3, 401),
    'maxpool/2x2_c4': _P(_pool, 'maxpool/2x2_c4', 2, 2, 2, 4, 402),
    'maxpool/6x10_c3': _P(_pool, 'maxpool/6x10_c3', 2, 6, 10, 3, 403),
    'maxpool/6x10_c4': _P(_pool, 'maxpool/6x10_c4', 2, 6, 10, 4, 404),
    'maxpool/6x10_c32': _P(_pool, 'maxpool/6x10_c32', 3, 6, 10, 32, 405),
    'maxpool/6x10_c4_offset_view': _P(_pool, 'maxpool/6x10_c4_offset_view', 2, 6, 10, 4, 406, offset=True),
    'maxpool/scalar_grid_loops': _P(_pool, 'maxpool/scalar_grid_loops', 1, 1400, 2000, 3, 407),
    'maxpool/vector_grid_loops': _P(_pool, 'maxpool/vector_grid_loops', 1, 2900, 2900, 4, 408),
    'maxpool/ties_c3': _P(_pool_ties, 'maxpool/ties_c3', 3),
    'maxpool/ties_c4': _P(_pool_ties, 'maxpool/ties_c4', 4),
    'maxpool/odd_5x7_c3': _P(_pool, 'maxpool/odd_5x7_c3', 2, 5, 7, 3, 411),
    'maxpool/odd_5x7_c4': _P(_pool, 'maxpool/odd_5x7_c4', 2, 5, 7, 4, 412),
    'maxpool/odd_7x4_c4': _P(_pool, 'maxpool/odd_7x4_c4', 2, 7, 4, 4, 413),
    'maxpool/odd_1x6_c4_empty': _P(_pool, 'maxpool/odd_1x6_c4_empty', 2, 1, 6, 4, 414),
    'maxpool/odd_13x13_c32': _P(_pool, 'maxpool/odd_13x13_c32', 2, 13, 13, 32, 415),
    'upsample/f1_c1': _P(_upsample, 'upsample/f1_c1', 2, 3, 5, 1, 1, 421),
    'upsample/f2_c6': _P(_upsample, 'upsample/f2_c6', 2, 5, 3, 6, 2, 422),
    'upsample/f3_c6': _P(_upsample, 'upsample/f3_c6', 2, 4, 7, 6, 3, 423),
    'upsample/f3_c1': _P(_upsample, 'upsample/f3_c1', 1, 7, 2, 1, 3, 424),
    'upsample/over_the_grid_cap': _P(_upsample, 'upsample/over_the_grid_cap', 1, 600, 700, 6, 2, 425),
    'tanh/range': _P(_tanh, 'tanh/range', 431),
    'yolo_head/10_43': _P(_head, 'yolo_head/10_43', 3 * 19 * 19, 10, 43, 441),
    'yolo_head/split0': _P(_head, 'yolo_head/split0', 50, 0, 5, 442),
    'yolo_head/no_classes': _P(_head, 'yolo_head/no_classes', 50, 10, 0, 443),
    'yolo_head/one_class': _P(_head, 'yolo_head/one_class', 300, 5, 1, 444),
    'yolo_head/logits_80': _P(_head, 'yolo_head/logits_80', 261, 10, 3, 445, big=80.0),
    'yolo_head/logits_100': _P(_head, 'yolo_head/logits_100', 261, 10, 3, 446, big=100.0),
    'permute/nchw_to_nhwc_c1': _P(_permute, 'permute/nchw_to_nhwc_c1', 'nchw_to_nhwc', (2, 1, 5, 7), 451),
    'permute/nchw_to_nhwc_c3': _P(_permute, 'permute/nchw_to_nhwc_c3', 'nchw_to_nhwc', (2, 3, 5, 7), 452),
    'permute/nchw_to_nhwc_c32': _P(_permute, 'permute/nchw_to_nhwc_c32', 'nchw_to_nhwc', (2, 32, 3, 5), 453),
    'permute/nhwc_to_nchw_c1': _P(_permute, 'permute/nhwc_to_nchw_c1', 'nhwc_to_nchw', (2, 7, 5, 1), 454),
    'permute/nhwc_to_nchw_c3': _P(_permute, 'permute/nhwc_to_nchw_c3', 'nhwc_to_nchw', (2, 7, 5, 3), 455),
    'permute/nhwc_to_nchw_c32': _P(_permute, 'permute/nhwc_to_nchw_c32', 'nhwc_to_nchw', (2, 3, 5, 32), 456),
    'permute/primary_caps_rows': _P(_permute, 'permute/primary_caps_rows', 'primary_caps_rows', (2, 3, 5, 32), 457, n_caps=8),
    'permute/primary_caps_rows_one_cap': _P(_permute, 'permute/primary_caps_rows_one_cap', 'primary_caps_rows', (2, 5, 3, 3), 458, n_caps=1),
    'permute/nchw_to_nhwc_over_the_grid_cap': _P(_permute, 'permute/nchw_to_nhwc_over_the_grid_cap', 'nchw_to_nhwc', (1, 3, 900, 800), 459),
    'pick/5x43x16': _P(_pick, 'pick/5x43x16', 5, 43, 16, 461),
    'pick/d1': _P(_pick, 'pick/d1', 7, 4, 1, 462),
    'pick/one_class': _P(_pick, 'pick/one_class', 3, 1, 16, 463),
    'pick/over_one_block': _P(_pick, 'pick/over_one_block', 40, 43, 16, 464),
}
FACTORY.update(_reduce_cases())
FACTORY['bn_param_grad/n257'] = lambda: dict(_red_fold('bn_param_grad/n257', 257, 1, 1.0, 267), kind='bn_param_grad')

_cache = {}


def case(name):
    if name in _cache:
        return _cache[name]
    c = FACTORY[name]()
    assert c['name'] == name
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    if name not in BIG:
        _cache[name] = c
    return c


def names(kind=None, big=None):
    """Case names, by kind (the part of the name in front of the slash) and, if given, by whether they are among the large ones."""
    return [n for n in FACTORY if (kind is None or n.split('/')[0] == kind) and (big is None or (n in BIG) == big)]


# the cases above the grid cap of stream_grid (65536 blocks of 256 threads): generated and checked on the device
# (tests/test_gpu_streaming.py); n4 = P N / 4 float4, `unroll` float4 a thread and pass of the unrolled body
ABOVE_CAP = {
    'affine_act': dict(N=256, P=9 * STREAM_CAP * 256 * 4 // 256 + 1000, unroll=4),
    'bn_bwd_apply': dict(N=256, P=5 * STREAM_CAP * 256 * 4 // 256 + 1000, unroll=2),
}


# ------------------------------------------------------------------------------------------------ the reference
def _lrelu(y, slope):
    return np.where(y > 0, y, y * slope)


MUTANTS = ('pool: row stride 2 Wo on an odd map', 'pool: tie goes to the last position', 'lrelu derivative on z', 'unbiased variance normalises',
           'running variance from the biased one', 'count == 1 divides by zero', 'variance not clamped', 'apply: xhat m2 dropped',
           'apply: m1 and m2 swapped', 'channel (4 tid) mod N', 'fold: b without running_mean', 'softmax without max subtraction',
           'softmax backward without the dot term', 'upsample backward sums f terms', 'tanh backward on x', 'permute: scatter equal to gather',
           'pick backward writes every class', 'act_bwd: zero takes the positive branch')


class Ref(object):
    """The operations from their definitions in numpy.  f = np.float64: the reference.  f = np.float32: the same formulas in float32
    (what the C-ABI holds in double stays double).  mutant: one named, plausible kernel bug."""

    def __init__(self, f=np.float64, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.f, self.mutant = f, mutant

    def _c(self, a):
        return None if a is None else np.asarray(a).astype(self.f)

    def _channels(self, P, N):
        """The channel of every element of a [P, N] tensor; None: the column, as it should be."""
        if self.mutant == 'channel (4 tid) mod N' and N % 4 == 0:      # the hoisted kernels' register trick where it does not hold
            e = np.arange(P * N).reshape(P, N)
            return ((e // 4) % 256 * 4) % N + e % 4
        return None

    def _per(self, v, ch):
        """A per-channel vector at every element of [P, N]."""
        v = self._c(v)
        return v[None, :] if ch is None else v[ch]

    # ---- csrc/bn.hip
    def bn_finalize(self, c):
        f, count = self.f, float(c['count'])
        s = c['stats'].sum(0)                                           # double sums: double in every evaluation
        m = s[:, 0] / count
        var = s[:, 1] / count - m * m                                   # the biased variance, from the sums
        if self.mutant != 'variance not clamped':
            var = np.maximum(var, 0.0)                                  # a variance is not negative
        if count > 1 or self.mutant == 'count == 1 divides by zero':
            with np.errstate(invalid='ignore', divide='ignore'):
                unbiased = var * count / (count - 1.0)
        else:
            unbiased = var
        if self.mutant == 'running variance from the biased one':
            unbiased = var
        norm_var = unbiased if self.mutant == 'unbiased variance normalises' else var
        with np.errstate(invalid='ignore'):
            invstd = (f(1.0) / np.sqrt(norm_var.astype(f) + f(c['eps']))).astype(f)
        gamma, beta, mom = self._c(c['gamma']), self._c(c['beta']), f(c['momentum'])
        mean = m.astype(f)
        scale = gamma * invstd
        out = dict(mean=mean, invstd=invstd, scale=scale, shift=beta - mean * scale, nbt=np.int64(c['nbt'] + 1))
        mag = {'mean': np.abs(m), 'invstd': invstd, 'scale': np.abs(scale), 'shift': np.abs(beta) + np.abs(mean * scale)}
        if c['running_mean'] is not None:
            rm, rv = self._c(c['running_mean']), self._c(c['running_var'])
            out['running_mean'] = (f(1) - mom) * rm + mom * mean
            out['running_var'] = (f(1) - mom) * rv + mom * unbiased.astype(f)
            mag['running_mean'] = np.abs((1 - mom) * rm) + np.abs(mom * mean)
            mag['running_var'] = np.abs((1 - mom) * rv) + np.abs(mom * unbiased)
        return _with_mag(out, mag)

    def bn_eval(self, c):
        f = self.f
        sc = self._c(c['gamma']) / np.sqrt(self._c(c['running_var']) + f(c['eps']))
        rm, beta = self._c(c['running_mean']), self._c(c['beta'])
        return _with_mag(dict(scale=sc, shift=beta - rm * sc), {'scale': np.abs(sc), 'shift': np.abs(beta) + np.abs(rm * sc)})

    def bn_fold(self, c):
        f = self.f
        sc = self._c(c['gamma']) / np.sqrt(self._c(c['running_var']) + f(c['eps']))
        W, rm, beta = self._c(c['W']), self._c(c['running_mean']), self._c(c['beta'])
        b = self._c(c['bias']) if c['bias'] is not None else np.zeros_like(rm)
        if self.mutant == 'fold: b without running_mean':
            rm = np.zeros_like(rm)
        return _with_mag(dict(Wf=W * sc[:, None], bf=(b - rm) * sc + beta),
                         {'Wf': np.abs(W * sc[:, None]), 'bf': (np.abs(b) + np.abs(rm)) * np.abs(sc) + np.abs(beta)})

    def _arg(self, c):
        """(y, |terms of y|): the LeakyReLU argument z scale + shift of a [P, N] case."""
        z = self._c(c['z'])
        if c['scale'] is None:
            return z, np.abs(z)
        ch = self._channels(c['P'], c['N'])
        sc, sh = self._per(c['scale'], ch), self._per(c['shift'], ch)
        return z * sc + sh, np.abs(z * sc) + np.abs(sh)

    def affine_act(self, c):
        y, mag = self._arg(c)
        slope = self.f(c['slope'])
        return _with_mag(dict(a=_lrelu(y, slope)), {'a': mag * np.where(y > 0, 1.0, slope)})

    def _masked(self, c):
        """(d, xhat, channels): the gradient behind the LeakyReLU and the normalised z."""
        y, _ = self._arg(c)
        z, g = self._c(c['z']), self._c(c['da'])
        on = (z if self.mutant == 'lrelu derivative on z' else y) > 0
        d = np.where(on, g, g * self.f(c['slope']))
        ch = self._channels(c['P'], c['N'])
        return d, (z - self._per(c['mean'], ch)) * self._per(c['invstd'], ch), ch

    def bn_bwd_reduce(self, c):
        d, xh, _ = self._masked(c)
        t = d * xh
        red = np.stack([d.astype(np.float64).sum(0), t.astype(np.float64).sum(0)], axis=1)
        return _with_mag(dict(red=red), {'red': np.stack([np.abs(d).astype(np.float64).sum(0), np.abs(t).astype(np.float64).sum(0)], axis=1)})

    def bn_bwd_apply(self, c):
        d, xh, ch = self._masked(c)
        means = (c['red'] * (1.0 / c['P'])).astype(self.f)              # double sums / the pixel count, then the float type
        m1, m2 = self._per(means[:, 0], ch), self._per(means[:, 1], ch)
        if self.mutant == 'apply: m1 and m2 swapped':
            m1, m2 = m2, m1
        if self.mutant == 'apply: xhat m2 dropped':
            m2 = np.zeros_like(m2)
        sc = self._per(c['scale'], ch)
        out = dict(dz=sc * (d - m1 - xh * m2))
        mag = {'dz': np.abs(sc) * (np.abs(d) + np.abs(m1) + np.abs(xh * m2))}
        if c['param_grads']:
            out.update(dbeta=c['red'][:, 0].astype(self.f), dgamma=c['red'][:, 1].astype(self.f))
            mag.update(dbeta=np.abs(c['red'][:, 0]), dgamma=np.abs(c['red'][:, 1]))
        return _with_mag(out, mag)

    def bn_red_fold(self, c):
        s = c['red_copies'].sum(0) * c['scale']
        a = np.abs(c['red_copies']).sum(0) * abs(c['scale'])
        out, mag = {}, {}
        for on, key, v, m in zip(c['outs'], ('red_out', 'dgamma', 'dbeta'), (s, s[:, 1].astype(self.f), s[:, 0].astype(self.f)),
                                 (a, a[:, 1], a[:, 0])):
            if on:
                out[key], mag[key] = v, m
        return _with_mag(out, mag)

    def bn_param_grad(self, c):
        red = c['red_copies'][0]
        return _with_mag(dict(dbeta=red[:, 0].astype(self.f), dgamma=red[:, 1].astype(self.f)),
                         dict(dbeta=np.abs(red[:, 0]), dgamma=np.abs(red[:, 1])))

    def act_bwd(self, c):
        z, g, slope = self._c(c['z']), self._c(c['da']), self.f(c['slope'])
        on = z >= 0 if self.mutant == 'act_bwd: zero takes the positive branch' else z > 0
        return _with_mag(dict(dz=np.where(on, g, g * slope)), {'dz': np.abs(g) * np.where(on, 1.0, slope)})

    def channel_sum(self, c):
        dz = self._c(c['dz'])
        return _with_mag(dict(out=dz.sum(0, dtype=self.f)), {'out': np.abs(c['dz']).sum(0)})

    # ---- csrc/misc.hip
    def maxpool(self, c):
        x, g = self._c(c['x']), self._c(c['g'])
        B, H, W, C = x.shape
        Ho, Wo = H // 2, W // 2
        dx = np.zeros_like(x)
        if Ho == 0 or Wo == 0:
            return dict(y=np.zeros((B, Ho, Wo, C), dtype=self.f), dx=dx)
        if self.mutant == 'pool: row stride 2 Wo on an odd map':       # the input walked as [B][2 Ho][2 Wo][C], whatever its shape is
            b, oy, ox, ch = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), np.arange(C), indexing='ij')
            base = ((b * (2 * Ho) + 2 * oy) * (2 * Wo) + 2 * ox) * C + ch
            where = [base, base + C, base + 2 * Wo * C, base + 2 * Wo * C + C]
            w = np.stack([x.reshape(-1)[i] for i in where])
        else:
            w = windows(x)
        best, bi = w[0].copy(), np.zeros(w[0].shape, dtype=np.int64)
        for k in (1, 2, 3):                                             # the first of equals wins: only a larger value takes over
            take = w[k] >= best if self.mutant == 'pool: tie goes to the last position' else w[k] > best
            best, bi = np.where(take, w[k], best), np.where(take, k, bi)
        if self.mutant == 'pool: row stride 2 Wo on an odd map':
            for k in range(4):
                dx.reshape(-1)[where[k]] = np.where(bi == k, g, 0.0)
        else:
            for k, (dy, dx_) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
                dx[:, dy:2 * Ho:2, dx_:2 * Wo:2] = np.where(bi == k, g, 0.0)
        return dict(y=best, dx=dx)

    def upsample(self, c):
        x, g, f = self._c(c['x']), self._c(c['g']), c['f']
        B, H, W, C = x.shape
        g6 = g.reshape(B, H, f, W, f, C)
        if self.mutant == 'upsample backward sums f terms':
            g6 = g6[:, :, :1]
        return dict(y=x.repeat(f, axis=1).repeat(f, axis=2), dx=g6.sum(axis=(2, 4), dtype=self.f))

    def tanh(self, c):
        x, g = self._c(c['x']), self._c(c['g'])
        y = np.tanh(x)
        t = x if self.mutant == 'tanh backward on x' else y
        return _with_mag(dict(y=y, dx=g * (1 - t * t)), dict(y=np.abs(y), dx=np.abs(g) * (1 + y * y)))

    def yolo_head(self, c):
        x, g, split, C = self._c(c['x']), self._c(c['g']), c['split'], c['C']
        f = self.f
        with np.errstate(over='ignore', invalid='ignore', under='ignore'):
            sig = f(1) / (f(1) + np.exp(-x[:, :split]))
            lg = x[:, split:]
            if C and self.mutant != 'softmax without max subtraction':
                lg = lg - lg.max(axis=1, keepdims=True)
            e = np.exp(lg)
            sm = e / e.sum(axis=1, keepdims=True) if C else e
        gs, gc = g[:, :split], g[:, split:]
        dot = (gc * sm).sum(axis=1, keepdims=True)
        if self.mutant == 'softmax backward without the dot term':
            dot = np.zeros_like(dot)
        y = np.concatenate([sig, sm], axis=1)
        dx = np.concatenate([gs * sig * (1 - sig), sm * (gc - dot)], axis=1)
        mag_dx = np.concatenate([np.abs(gs * sig) * (1 + sig), sm * (np.abs(gc) + np.abs(gc * sm).sum(axis=1, keepdims=True))], axis=1)
        return _with_mag(dict(y=y, dx=dx), dict(y=np.abs(y) + 1e-30, dx=mag_dx + 1e-30))      # 1e-30: below it float32 has run out of range

    def permute(self, c):
        x, op = self._c(c['x']), c['op']
        src = np.arange(x.size).reshape(x.shape)
        if op == 'nchw_to_nhwc':
            fwd = lambda a: a.transpose(0, 2, 3, 1)
        elif op == 'nhwc_to_nchw':
            fwd = lambda a: a.transpose(0, 3, 1, 2)
        else:                       # [B,H,W,(o,cap)] -> [B, o H W + y W + x, cap]: the view(B, -1, 1) + cat of the n_caps NCHW convolutions
            B, H, W, Cc = x.shape
            fwd = lambda a: a.reshape(B, H, W, Cc // c['n_caps'], c['n_caps']).transpose(0, 3, 1, 2, 4).reshape(B, -1, c['n_caps'])
        y = np.ascontiguousarray(fwd(x))
        out = dict(y=y)
        if c.get('g') is not None:
            j = np.ascontiguousarray(fwd(src)).reshape(-1)              # y.flat[i] = x.flat[j[i]]
            g = self._c(c['g']).reshape(-1)
            dx = np.zeros(x.size, dtype=self.f)
            if self.mutant == 'permute: scatter equal to gather':
                dx[:] = g[j]
            else:
                dx[j] = g
            out['dx'] = dx.reshape(x.shape)
        return out

    def pick(self, c):
        caps, y, g = self._c(c['caps']), c['y'], self._c(c['g'])
        rows = np.arange(caps.shape[0])
        dcaps = np.zeros_like(caps)
        if self.mutant == 'pick backward writes every class':
            dcaps[:] = g[:, None, :]
        else:
            dcaps[rows, y] = g
        return dict(out=caps[rows, y], dcaps=dcaps)


def _with_mag(out, mag):
    for k, v in mag.items():
        out['mag:' + k] = np.asarray(v, dtype=np.float64)
    return out


EXACT_KINDS = ('maxpool', 'upsample', 'permute', 'pick')
SUM_KINDS = ('bn_bwd_reduce',)


def run(c, impl):
    return getattr(impl, c['kind'])(c)


_refs = {}


def reference(name, f=np.float64):
    """The reference's result of a case in float64 (or its float32 evaluation): computed once for the small cases, never changed."""
    key = (name, np.dtype(f).name)
    if key in _refs:
        return _refs[key]
    ref = run(case(name), Ref(f))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    if name in BIG:
        for k in [k for k in _refs if k[0] in BIG and k[0] != name]:   # one large case at a time
            del _refs[k]
    _refs[key] = ref
    return ref


def mode(c, key):
    if key == 'nbt' or c.get('exact') or c['kind'] in EXACT_KINDS:
        return 'exact'
    return 'sum' if c['kind'] in SUM_KINDS else 'rule'


def _same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return False
    if ref.dtype.kind in 'iu' or got.dtype.kind in 'iu':
        return bool(np.array_equal(got.astype(np.int64), ref.astype(np.int64)))
    t = np.float64 if got.dtype == np.float64 and ref.dtype == np.float64 else np.float32
    return np.ascontiguousarray(got, dtype=t).tobytes() == np.ascontiguousarray(ref, dtype=t).tobytes()


def _rel(got, ref, mag):
    """Largest |got - ref| / mag; where mag is 0 the value must be the reference's; inf for a wrong shape, a NaN or an infinity."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return float('inf')
    err = np.abs(got - ref)
    zero = mag == 0
    if (err[zero] != 0).any():
        return float('inf')
    if zero.all():
        return 0.0
    return float((err[~zero] / mag[~zero]).max())


def fractions(c, got):
    """Every output's largest error as a fraction of its tolerance (0 or inf for the exact ones): {output: fraction}."""
    ref, ref32 = reference(c['name']), reference(c['name'], np.float32)
    keys = sorted(k for k in ref if not k.startswith('mag:'))
    assert sorted(k for k in got if not k.startswith('mag:')) == keys, (sorted(got), keys)
    out = {}
    for k in keys:
        m = mode(c, k)
        if m == 'exact':
            out[k] = 0.0 if _same_bits(got[k], ref[k]) else float('inf')
            continue
        mag = ref['mag:' + k]
        e = _rel(got[k], ref[k], mag)
        tol = 1e-6 if m == 'sum' else max(1e-6, 20.0 * _rel(ref32[k], ref[k], mag))
        out[k] = e / tol
    return out


def compare(c, got):
    """Assert that `got` is the reference's result of the case within the tolerances of this file's header; returns the fractions."""
    fr = fractions(c, got)
    bad = dict((k, v) for k, v in fr.items() if not v <= 1.0)
    assert not bad, '%s: outside the tolerance (error / tolerance): %s' % (c['name'], bad)
    return fr


def accepts(c, got):
    try:
        compare(c, got)
        return True
    except AssertionError:
        return False


# ------------------------------------------------------------------------------------------------ the kernels
class Kernels(object):
    """The thin adapter: every case through capsyolo_amd._lib.call or capsyolo_amd.ops on the GPU.  Outputs start as NaN (fresh NaN
    buffers for the direct calls; the allocator's free blocks are filled with NaN in front of the ops calls), so an element that a kernel
    leaves unwritten shows."""

    def __init__(self):
        import torch
        from capsyolo_amd import ops
        from capsyolo_amd._lib import call
        self.torch, self.ops, self.call = torch, ops, call

    def st(self):
        return self.torch.cuda.current_stream().cuda_stream

    def dev(self, a, dtype=None, offset=False):
        """A device copy (float32 unless told); offset: a contiguous view that starts one element into its buffer (not 16-byte aligned)."""
        if a is None:
            return None
        torch = self.torch
        dtype = dtype or torch.float32
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        if not offset:
            return t.cuda()
        buf = torch.empty(t.numel() + 1, dtype=dtype, device='cuda')
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    def nan(self, shape, dtype=None, offset=False):
        torch = self.torch
        n = int(np.prod(shape))
        buf = torch.full((n + (1 if offset else 0),), float('nan'), dtype=dtype or torch.float32, device='cuda')
        return (buf[1:] if offset else buf).view(shape)

    def poison(self, *shapes):
        """Blocks of the sizes the ops wrappers are about to allocate, filled with NaN and freed: torch.empty hands them out again."""
        held = [self.torch.full(tuple(s), float('nan'), device='cuda') for s in shapes for _ in range(2) if int(np.prod(s))]
        self.torch.cuda.synchronize()
        del held

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()

    @staticmethod
    def host(**tensors):
        return dict((k, v.detach().cpu().numpy()) for k, v in tensors.items())

    def bn_finalize(self, c):
        torch, N = self.torch, c['N']
        stats = self.dev(c['stats'], torch.float64)
        gamma, beta = self.dev(c['gamma']), self.dev(c['beta'])
        rm, rv = self.dev(c['running_mean']), self.dev(c['running_var'])
        nbt = torch.tensor(c['nbt'], dtype=torch.long, device='cuda')
        o = dict((k, self.nan((N,))) for k in ('scale', 'shift', 'mean', 'invstd'))
        self.call('cy_bn_finalize', self.p(stats), c['count'], self.p(gamma), self.p(beta), self.p(rm), self.p(rv), c['momentum'], c['eps'],
                  self.p(o['scale']), self.p(o['shift']), self.p(o['mean']), self.p(o['invstd']), N, self.p(nbt), self.st())
        o['nbt'] = nbt
        if rm is not None:
            o.update(running_mean=rm, running_var=rv)
        return self.host(**o)

    def bn_eval(self, c):
        N = c['N']
        t = [self.dev(c[k]) for k in ('gamma', 'beta', 'running_mean', 'running_var')]
        scale, shift = self.nan((N,)), self.nan((N,))
        self.call('cy_bn_eval_scale_shift', *[self.p(v) for v in t], c['eps'], self.p(scale), self.p(shift), N, self.st())
        return self.host(scale=scale, shift=shift)

    def bn_fold(self, c):
        t = [self.dev(c[k]) for k in ('W', 'bias', 'gamma', 'beta', 'running_mean', 'running_var')]
        Wf, bf = self.nan(c['W'].shape), self.nan((c['Cout'],))
        self.call('cy_bn_fold_eval', *[self.p(v) for v in t], c['eps'], self.p(Wf), self.p(bf), c['Cout'], c['per_out'], self.st())
        return self.host(Wf=Wf, bf=bf)

    def affine_act(self, c):
        z = self.dev(c['z'], offset=c['offset'])
        a = self.nan(c['z'].shape, offset=c['offset'])
        scale, shift = self.dev(c['scale']), self.dev(c['shift'])
        self.call('cy_affine_act', self.p(z), self.p(a), self.p(scale), self.p(shift), c['slope'], c['P'], c['N'], self.st())
        return self.host(a=a)

    def _bwd_inputs(self, c):
        return [self.dev(c[k]) for k in ('z', 'da')], [self.dev(c[k]) for k in ('scale', 'shift', 'mean', 'invstd')]

    def bn_bwd_reduce(self, c):
        (z, da), ch = self._bwd_inputs(c)
        red = self.nan((c['N'], 2), self.torch.float64)
        self.call('cy_bn_bwd_reduce', self.p(z), self.p(da), *[self.p(v) for v in ch], c['slope'], self.p(red), c['P'], c['N'], self.st())
        return self.host(red=red)

    def bn_bwd_apply(self, c):
        (z, da), ch = self._bwd_inputs(c)
        red = self.dev(c['red'], self.torch.float64)
        dz = self.nan(c['z'].shape)
        dgamma, dbeta = (self.nan((c['N'],)), self.nan((c['N'],))) if c['param_grads'] else (None, None)
        self.call('cy_bn_bwd_apply', self.p(z), self.p(da), self.p(dz), *[self.p(v) for v in ch], None, c['slope'], self.p(red), self.p(dgamma),
                  self.p(dbeta), c['P'], c['N'], self.st())
        out = dict(dz=dz)
        if c['param_grads']:
            out.update(dgamma=dgamma, dbeta=dbeta)
        return self.host(**out)

    def bn_red_fold(self, c):
        f64, N = self.torch.float64, c['N']
        src = self.dev(c['red_copies'], f64)
        on_out, on_g, on_b = c['outs']
        out = (src.view(-1)[:2 * N].view(N, 2) if c['inplace'] else self.nan((N, 2), f64)) if on_out else None
        dgamma, dbeta = self.nan((N,)) if on_g else None, self.nan((N,)) if on_b else None
        self.call('cy_bn_red_fold', self.p(src), c['copies'], c['scale'], self.p(out), self.p(dgamma), self.p(dbeta), N, self.st())
        named = dict(red_out=out, dgamma=dgamma, dbeta=dbeta)
        return self.host(**dict((k, v) for k, v in named.items() if v is not None))

    def bn_param_grad(self, c):
        N = c['N']
        red = self.dev(c['red_copies'][0], self.torch.float64)
        dgamma, dbeta = self.nan((N,)), self.nan((N,))
        self.call('cy_bn_param_grad', self.p(red), self.p(dgamma), self.p(dbeta), N, self.st())
        return self.host(dgamma=dgamma, dbeta=dbeta)

    def act_bwd(self, c):
        z, da, dz = self.dev(c['z']), self.dev(c['da']), self.nan((c['n'],))
        self.call('cy_act_bwd', self.p(z), self.p(da), self.p(dz), c['slope'], c['n'], self.st())
        return self.host(dz=dz)

    def channel_sum(self, c):
        dz, out = self.dev(c['dz']), self.nan((c['N'],))
        self.call('cy_channel_sum', self.p(dz), self.p(out), c['P'], c['N'], self.st())
        return self.host(out=out)

    def _through_ops(self, fn, x, g, offset=False):
        """y = fn(x) and the gradient of x for the output gradient g, through the autograd wrappers of capsyolo_amd.ops."""
        xd = self.dev(x, offset=offset).requires_grad_(True)
        gd = self.dev(g, offset=offset)
        self.poison(g.shape, g.shape)
        y = fn(xd)
        assert tuple(y.shape) == tuple(g.shape), (tuple(y.shape), g.shape)
        self.poison(x.shape, x.shape)
        y.backward(gd)
        return y, xd.grad

    def maxpool(self, c):
        y, dx = self._through_ops(self.ops.maxpool2, c['x'], c['g'], c['offset'])
        return self.host(y=y, dx=dx)

    def upsample(self, c):
        y, dx = self._through_ops(lambda x: self.ops.upsample_nearest(x, c['f']), c['x'], c['g'])
        return self.host(y=y, dx=dx)

    def tanh(self, c):
        y, dx = self._through_ops(self.ops.tanh, c['x'], c['g'])
        return self.host(y=y, dx=dx)

    def yolo_head(self, c):
        y, dx = self._through_ops(lambda x: self.ops.yolo_head(x, c['split'], c['C']), c['x'], c['g'])
        return self.host(y=y, dx=dx)

    def permute(self, c):
        fn = getattr(self.ops, c['op'])
        y, dx = self._through_ops((lambda x: fn(x, c['n_caps'])) if c['n_caps'] else fn, c['x'], c['g'])
        return self.host(y=y, dx=dx)

    def pick(self, c):
        labels = self.torch.from_numpy(c['y']).cuda()
        out, dcaps = self._through_ops(lambda x: self.ops.pick_capsule(x, labels), c['caps'], c['g'])
        return self.host(out=out, dcaps=dcaps)

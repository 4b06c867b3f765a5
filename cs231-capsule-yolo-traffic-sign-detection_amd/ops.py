"""torch.autograd wrappers over the C-ABI kernels (include/capsyolo_hip.h).

PyTorch supplies device memory, the current HIP stream and the autograd graph; every
arithmetic step below is a call into libcapsyolo_hip.so.  All activations are NHWC fp32
tensors ([B,H,W,C], plain contiguous).  No function here has a CPU or ATen fallback.
"""
import collections
import ctypes as C
import functools

import torch

from . import _lib
from ._lib import ConvGemm, ConvWgrad, RoutingBwd, RoutingFwd, call, query


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer(object):
    """HIP-event brackets around selected launches on the stream they are launched on (bench.py's live
    per-kernel durations).  Disabled by default: then ``range`` costs one attribute test."""

    def __init__(self):
        self.enabled = False
        self.events = {}

    class _Range(object):
        def __init__(self, timer, name):
            self.timer, self.name = timer, name

        def __enter__(self):
            if self.timer.enabled:
                self.start = torch.cuda.Event(enable_timing=True)
                self.start.record(torch.cuda.current_stream())

        def __exit__(self, *exc):
            if self.timer.enabled:
                end = torch.cuda.Event(enable_timing=True)
                end.record(torch.cuda.current_stream())
                self.timer.events.setdefault(self.name, []).append((self.start, end))
            return False

    def range(self, name):
        return KernelTimer._Range(self, name)

    def reset(self):
        self.events = {}

    def summary(self):
        """name -> (launches, mean milliseconds); call after a device synchronize."""
        return dict((k, (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v))) for k, v in self.events.items())


timer = KernelTimer()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t, name='tensor'):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise _lib.HipExtensionError('%s must be a float32 tensor on the GPU (got %s on %s); there is no CPU fallback'
                                     % (name, t.dtype, t.device))
    return t if t.is_contiguous() else t.contiguous()


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


class _ZeroPool(object):
    """Scratch that must start at zero (BatchNorm statistics and backward sums are accumulated with atomics): slices of
    one arena per device that is zeroed by ONE cy_zero_bytes launch per training step (FusedBackbone.forward calls
    reset()), instead of one fill kernel per buffer (~23 per step at the headline model)."""

    def __init__(self):
        self.pools = {}

    def reset(self, device):
        st = self.pools.get(device)
        if st is None:
            return
        if st['need'] > st['buf'].numel():                       # grow: the new arena is born zeroed
            st['buf'] = torch.zeros(2 * st['need'], dtype=torch.uint8, device=device)
        elif st['off']:
            call('cy_zero_bytes', C.c_void_p(st['buf'].data_ptr()), st['off'], _stream())
        st['off'], st['need'] = 0, 0

    def take(self, shape, dtype, device):
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = (n * torch.empty((), dtype=dtype).element_size() + 255) & ~255
        st = self.pools.get(device)
        if st is None:
            st = self.pools[device] = {'buf': torch.zeros(1 << 20, dtype=torch.uint8, device=device), 'off': 0, 'need': 0}
        st['need'] += nbytes
        if st['off'] + nbytes > st['buf'].numel():               # arena exhausted: a fresh fill now, a larger arena next step
            return torch.zeros(shape, dtype=dtype, device=device)
        out = st['buf'][st['off']:st['off'] + nbytes].view(dtype)[:n].view(shape)
        st['off'] += nbytes
        return out


zero_pool = _ZeroPool()
_zero_consts = {}


def _const_zeros(n, like):
    """A shared, never-written vector of zeros: the gradient of a conv bias in front of BatchNorm (analytically 0)."""
    key = (int(n), like.device)
    t = _zero_consts.get(key)
    if t is None:
        t = _zero_consts[key] = torch.zeros(n, dtype=torch.float32, device=like.device)
    return t


# ------------------------------------------------------------------------------------------------ convolution
def _x_geometry(shape, nchw):
    if nchw:
        B, Cin, Hi, Wi = shape
        return B, Hi, Wi, Cin, (Cin * Hi * Wi, Wi, 1, Hi * Wi)
    B, Hi, Wi, Cin = shape
    return B, Hi, Wi, Cin, (Hi * Wi * Cin, Wi * Cin, Cin, 1)


STATS_COPIES = 16       # CY_STATS_COPIES of include/capsyolo_hip.h: BatchNorm statistics are accumulated in 16 striped copies
USE_CONV1_MOMENTS = True  # ... whose BatchNorm statistics come from the 28 x 28 moment matrix of the input patches (csrc/conv1_moments.hip)
USE_CONV1_ONEPASS = True  # ... and whose backward then needs ONE pass over the gradient (cy_conv1_bn_bwd_onepass)
CONV1_SIGNMASK = True     # ... which takes lrelu'(y) from one bit per element that the activation pass stored (cy_conv1_bn_bwd_onepass_mask: no z recomputed)
CONV1_MOMENTS_MIN_PIXELS = 1 << 18   # ... from this many pixels on: below, its three launches cost more than the one recompute pass saves
USE_CONV1_BWD = True     # ... and the backward of its whole conv -> BatchNorm -> LeakyReLU block without z / dz in memory
USE_CONV1 = True         # 3 -> {32, 64, 128} channels, 3x3, NCHW image (the backbones' first layer): dedicated store-bound kernels
USE_WINOGRAD_S2_DGRAD = True   # ... and their input gradient (K = Cout: short reductions; kept switchable)
USE_WINOGRAD_S2 = True   # 4x4 / stride 2 / pad 1 layers: fused Winograd F(2x2,2x2) forward on the space-to-depth view
USE_WINOGRAD = True      # 3x3 / stride 1 / pad 1 layers with Cin % 8 == 0 take the fused Winograd F(2x2,3x3) kernel
USE_WINOGRAD4_S2 = True  # 4x4 / stride-2 layers: forward on F(4x4,2x2) (winograd4_s2.hip: 1.44x fewer MFMAs than F(2x2,2x2)) from
USE_WINOGRAD4_S2_DGRAD = True      # ... and their input gradient (the same kernel over dY shifted by one pixel, scattered to the four classes)
WINOGRAD4_S2_MIN_PIXELS = 1 << 16   # this many output pixels on (its 16 x 32-pixel blocks are the F(2x2,2x2) kernel's)
USE_WINOGRAD4 = True     # ... forward and input gradient on F(4x4,3x3) (winograd4.hip: 1.78x fewer MFMAs) from WINOGRAD4_MIN_PIXELS output pixels on
WINOGRAD4_MIN_PIXELS = 1 << 17   # 512 output pixels x 64 channels per block: far below, its tile grid leaves most of the 256 CUs idle.  The value is a
                                 # trade of speed against LeakyReLU kink flips, measured in round 4 (tools/bench_darknet.py 16 <log2 pixels>): darknet_d
                                 # 8.83 ms per step at 2^18 (round 3's value), 8.69 at 2^17 / 2^16, 8.47 at 2^15, 8.44 at 2^13 -- but F(4x4,3x3) is 2.3e-6
                                 # from fp64 against 3.6e-7 for F(2x2,3x3), and on the 19-block net every further layer on it flips more pre-activations
                                 # inside the rounding noise: gradients of the lower blocks against an fp64 run of the same net (128 x 128, three seeds) 5e-3 / 4e-4 /
                                 # 5e-3 at 2^18 and 2e-2 / 9e-3 / 1.7e-2 at 2^15 (the reference's own fp32 path: 5e-6 / 3e-3 / 8e-3).  2^17 takes the
                                 # layers where the kernel buys most (>= 131072 output pixels) and leaves the deep small maps on F(2x2,3x3).


FUSE_BN_BWD_REDUCE = True  # ... and that block's input-gradient epilogue sums the producer's BatchNorm backward
FUSE_BN_BWD_APPLY = True   # 3x3 blocks whose weight gradient is the Winograd kernel: BatchNorm backward pass 2 inside that kernel
FUSE_INPUT_AFFINE = True  # a BN+LeakyReLU block in front of a 4x4/stride-2 block hands over its raw output + scale/shift
USE_WINOGRAD4_WGRAD = True   # the 3x3 layers' weight gradient on F(3x3,4x4) (winograd4_wgrad.hip) where its shape conditions hold and the
                             # map has WINOGRAD4_MIN_PIXELS output pixels (below, the F(3x3,2x2) kernel)

ConvPlan = collections.namedtuple('ConvPlan', [
    'fwd', 'dgrad', 'wgrad',   # the kernel family of each pass, named by its timer.range prefix (dgrad None: NCHW input, not implemented)
    'in_affine',               # forward AND weight gradient take the producer's BatchNorm + LeakyReLU on their input loads (4x4 / stride 2)
    'dgrad_bn_fuse',           # the input gradient's epilogue can sum the producer's BatchNorm backward (conv_dgrad's bn_fuse) ...
    'dgrad_premasks',          # ... and then stores dx * lrelu'(y), not dx (the 4x4 / stride-2 Winograd kernels, capsyolo_hip.h)
    'wgrad_bn',                # the weight gradient has the form with BatchNorm-backward pass 2 inside (conv_wino_wgrad_bn) ...
    'wgrad_bn4',               # ... and, for a premasked gradient only, its F(3x3,4x4) form (conv_wino4_wgrad_bn)
    'conv1',                   # a first-layer shape (csrc/conv1.hip: 3 -> {32, 64, 128} channels, 3x3 s1 p1, NCHW image)
    'conv1_bwd',               # ... whose training block runs without z / dz in memory
    'conv1_moments',           # ... taking its statistics from the moment matrix of the input patches
    'conv1_onepass',           # ... and, behind those statistics, its backward in one pass over the gradient
    'conv1_signmask'])         # ... that reads the sign of y from the forward's bit mask instead of recomputing z (fp32 block)
_WINO3_DGRAD = ('conv_wino_dgrad', 'conv_wino4_dgrad')


@functools.lru_cache(maxsize=None)
def _shape_ok(name, *shape):
    """One of the library's cy_*_ok host queries: a pure function of the shape, asked once per shape."""
    return bool(query(name, *shape))


def conv_plan(in_shape, cout, k, stride, pad, nchw=False, relu=False, lrelu=False):
    """Which kernel family runs each pass of one fp32 convolution, and what its block may fuse: a ConvPlan.  Host arithmetic
    on the shape (in_shape = x.shape: NCHW if nchw, else NHWC), the epilogue (relu: fused ReLU; lrelu: the eval-mode LeakyReLU
    epilogue) and the switches and thresholds above AS THEY STAND NOW -- every conv_forward / conv_dgrad / conv_wgrad / conv_block
    call asks again, nothing is cached across a switch change.  This is the only place that decides."""
    if nchw:
        B, Cin, Hi, Wi = in_shape
    else:
        B, Hi, Wi, Cin = in_shape
    fwd, dgrad, wgrad = 'conv_gemm_fwd', None if nchw else 'conv_gemm_dgrad', 'conv_wgrad'
    in_affine = wgrad_bn = wgrad_bn4 = conv1 = False
    if k == 3 and stride == 1 and pad == 1:
        px = B * Hi * Wi
        if nchw:
            conv1 = bool(USE_CONV1 and Cin == 3 and cout in (32, 64, 128) and Wi % 32 == 0)
            if conv1:
                fwd, wgrad = fwd if relu or lrelu else 'conv1_fwd', 'conv1_wgrad'
        elif USE_WINOGRAD:
            f4 = USE_WINOGRAD4 and px >= WINOGRAD4_MIN_PIXELS
            if not relu and Cin % 8 == 0 and Cin >= 8:
                fwd = 'conv_wino4_fwd' if f4 else 'conv_wino_fwd'
            if cout % 8 == 0 and cout >= 8:
                dgrad = 'conv_wino4_dgrad' if f4 else 'conv_wino_dgrad'
            w3 = Cin % 64 == 0 and cout % 64 == 0
            w4 = bool(USE_WINOGRAD4_WGRAD and px >= WINOGRAD4_MIN_PIXELS and _shape_ok('cy_wino4_wgrad_ok', B, Hi, Wi, Cin, cout))
            wgrad = 'conv_wino4_wgrad' if w4 else 'conv_wino_wgrad' if w3 else wgrad
            wgrad_bn = bool(FUSE_BN_BWD_APPLY and w3)
            wgrad_bn4 = wgrad_bn and w4
    elif (k == 4 and stride == 2 and pad == 1 and not nchw and USE_WINOGRAD and USE_WINOGRAD_S2 and Hi % 2 == 0 and Wi % 2 == 0):
        f4 = USE_WINOGRAD4_S2 and B * (Hi // 2) * (Wi // 2) >= WINOGRAD4_S2_MIN_PIXELS
        if not relu and Cin % 8 == 0:
            fwd = 'conv_wino42_fwd' if f4 and _shape_ok('cy_wino4s2_ok', B, Hi, Wi, Cin, cout) else 'conv_wino2_fwd'
        if USE_WINOGRAD_S2_DGRAD and Cin % 64 == 0 and cout % 8 == 0:
            dgrad = ('conv_wino42_dgrad' if f4 and USE_WINOGRAD4_S2_DGRAD and _shape_ok('cy_wino4s2_dgrad_ok', B, Hi, Wi, Cin, cout)
                     else 'conv_wino2_dgrad')
        if Cin % 32 == 0 and cout % 64 == 0:
            wgrad, in_affine = 'conv_wino2_wgrad', not relu
    dgrad_bn_fuse = bool(FUSE_BN_BWD_REDUCE and dgrad is not None and dgrad not in _WINO3_DGRAD and Cin % 4 == 0)
    conv1_bwd = bool(conv1 and USE_CONV1_BWD)
    conv1_moments = bool(conv1_bwd and USE_CONV1_MOMENTS and B * Hi * Wi >= CONV1_MOMENTS_MIN_PIXELS)
    conv1_onepass = bool(conv1 and USE_CONV1_ONEPASS)
    return ConvPlan(fwd, dgrad, wgrad, in_affine, dgrad_bn_fuse, dgrad_bn_fuse and dgrad in ('conv_wino2_dgrad', 'conv_wino42_dgrad'),
                    wgrad_bn, wgrad_bn4, conv1, conv1_bwd, conv1_moments, conv1_onepass,
                    bool(CONV1_SIGNMASK and conv1_moments and conv1_onepass))


ImageGradPlan = collections.namedtuple('ImageGradPlan', [
    'ok',                      # cy_conv_image_grad takes this first layer (Cin 3, stride 1, k odd up to 9, pad 0..k/2, Cout up to 1024)
    'family',                  # its timer.range prefix
    'tile',                    # (rows, columns) of image pixels per block
    'blocks',                  # blocks of the launch: B * ceil(H / 16) * ceil(W / 32)
    'chunks'])                 # passes over LDS: ceil(Cout / 8) chunks of dz channels
IMAGE_GRAD_TILE, IMAGE_GRAD_CK = (16, 32), 8      # IG_TY x IG_TX, IG_CK of csrc/image_grad.hip


def image_grad_plan(in_shape_nchw, cout, k, stride, pad):
    """Whether the gradient with respect to the NCHW image of one first layer is built (csrc/image_grad.hip), and the launch it
    takes: an ImageGradPlan.  Host arithmetic and the library's own cy_conv_image_grad_ok; conv_plan and ConvPlan know nothing of it
    (ConvPlan.dgrad stays None for an NCHW input: that field names the NHWC input-gradient kernels)."""
    B, Cin, Hi, Wi = (int(v) for v in in_shape_nchw)
    cout, k, stride, pad = int(cout), int(k), int(stride), int(pad)
    ok = bool(Cin == 3 and stride == 1 and _shape_ok('cy_conv_image_grad_ok', B, Hi, Wi, cout, k, pad))
    ty, tx = IMAGE_GRAD_TILE
    return ImageGradPlan(ok, 'conv_image_grad', IMAGE_GRAD_TILE, B * (-(-Hi // ty)) * (-(-Wi // tx)) if ok else 0,
                         -(-cout // IMAGE_GRAD_CK) if ok else 0)


def conv_image_grad(dy, weight, in_shape, k, pad, act=None, slope=1.0, scale=None, tag='conv'):
    """dx[B,3,H,W] (NCHW) of a stride-1 first layer from dy[B,Ho,Wo,Cout] (NHWC) and weight[Cout,3,k,k].  act: the block's own
    output, whose sign selects 1 or `slope` (in [0, 1]) as the activation's derivative; scale[Cout]: the eval-mode BatchNorm scale.
    Both are applied on the kernel's loads of dy (capsyolo_hip.h: cy_conv_image_grad); without them dy is the gradient dz itself."""
    dy, weight = _f32(dy, 'grad'), _f32(weight, 'conv weight')
    B, Cin, Hi, Wi = (int(v) for v in in_shape)
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, Cin, k, k) or tuple(dy.shape) != (B, Hi + 2 * pad - k + 1, Wi + 2 * pad - k + 1, Cout):
        raise _lib.HipExtensionError('conv_image_grad: dy %s and weight %s do not belong to a %dx%d / pad %d layer on an image %s'
                                     % (tuple(dy.shape), tuple(weight.shape), k, k, pad, (B, Cin, Hi, Wi)))
    if not image_grad_plan((B, Cin, Hi, Wi), Cout, k, 1, pad).ok:
        raise _lib.HipExtensionError('conv_image_grad: no kernel for image %s, Cout=%d, k=%d, pad=%d (built: 3 input channels, stride 1, '
                                     'k odd in 1..9, pad 0..k//2, Cout 1..1024)' % ((B, Cin, Hi, Wi), Cout, k, pad))
    if act is not None:
        act = _f32(act, 'activation')
        if tuple(act.shape) != tuple(dy.shape) or not 0.0 <= float(slope) <= 1.0:
            raise _lib.HipExtensionError('conv_image_grad: act %s must have the shape of dy %s and slope %r must lie in [0, 1]'
                                         % (tuple(act.shape), tuple(dy.shape), slope))
    if scale is not None:
        scale = _f32(scale, 'scale')
        if tuple(scale.shape) != (Cout,):
            raise _lib.HipExtensionError('conv_image_grad: scale %s must be [%d]' % (tuple(scale.shape), Cout))
    dx = _empty((B, Cin, Hi, Wi), dy)
    with timer.range('conv_image_grad/' + tag):
        call('cy_conv_image_grad', _ptr(dy), _ptr(act), _ptr(scale), _ptr(weight), _ptr(dx), B, Hi, Wi, Cin, Cout, k, pad, float(slope),
             _stream())
    return dx


BF16_DGRAD_ONE_LAUNCH = True       # bf16 path: the output-parity classes of a strided input gradient in one launch (cy_conv_gemm_bf16_classes)
FUSE_BN_BWD_REDUCE_BF16 = True     # bf16 path: the producer block's BatchNorm-backward sums out of the consumer's input-gradient epilogue
FUSE_BN_BWD_APPLY_BF16 = True      # bf16 path: BatchNorm-backward pass 2 inside the weight gradient (cy_conv_wgrad_bf16_bn) where the gradient arrives premasked

ConvPlanBF16 = collections.namedtuple('ConvPlanBF16', [
    'ok',                      # the bf16 kernels are built for this layer (FusedBackbone._forward_bf16 refuses every other)
    'fwd', 'dgrad', 'wgrad',   # the kernel family of each pass, named by its timer.range prefix (None where not ok)
    'dgrad_one_launch',        # the input gradient's output-parity classes go out together (cy_conv_gemm_bf16_classes)
    'dgrad_bn_fuse',           # the input gradient's epilogue can sum the producer's BatchNorm backward (conv_dgrad_bf16's bn_fuse) ...
    'dgrad_premasks',          # ... and then stores dx * lrelu'(y), not dx (the bf16 epilogue always does)
    'wgrad_bn',                # the weight gradient has the form with BatchNorm-backward pass 2 inside (conv_bf16_wgrad_bn)
    'launches'])               # {'fwd': [...], 'dgrad': [...]}: {BM, BN, TAPIN, ntiles, blocks} per launch; None where the library refuses the GEMM


def conv_plan_bf16(in_shape, cout, k, stride, pad, in_f32=False, out_f32=False):
    """The bf16 twin of conv_plan (in_shape = x's NHWC shape; in_f32: the input gradient leaves in fp32 for an fp32 producer; out_f32:
    the forward writes fp32).  Host arithmetic on the shape, the library's own answers for the descriptors the launches will carry,
    and the three switches above AS THEY STAND NOW: every call asks again.  What depends on the step stays at the use: whether a
    hand-over is there and fits (_input_grad), whether the gradient arrived premasked and in bf16 (_ConvBlockBF16.backward)."""
    B, Hi, Wi, Cin, xs = _x_geometry(in_shape, False)
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    # (k < stride leaves input pixels without taps: dgrad_classes refuses, there is no input gradient and launches['dgrad'] is [])
    classes, descs = _gemm_dgrad_descs(in_shape, (B, Ho, Wo, cout), k, stride, pad) if k >= stride else ((), ())
    sizes = set((c['TH'], c['TW'], c['Ho'], c['Wo']) for c in classes)
    one_launch = bool(BF16_DGRAD_ONE_LAUNCH and 1 < len(classes) <= 4 and len(sizes) == 1)      # (even maps: every class the same grid and taps)
    launches = {'fwd': _launches_bf16([_gemm_fwd_desc(B, Hi, Wi, Cin, xs, cout, k, stride, pad)], False, out_f32),
                'dgrad': _launches_bf16(descs, one_launch, in_f32)}
    ok = bool(pad == 1 and launches['fwd'] and launches['dgrad'] and query('cy_conv_wgrad_bf16_ws_floats', B, Ho, Wo, Cin, cout, k, stride) >= 0)
    wgrad_bn = bool(ok and FUSE_BN_BWD_APPLY_BF16 and query('cy_conv_wgrad_bf16_bn_ws_floats', B, Ho, Wo, Cin, cout, k, stride) >= 0)
    bn_fuse = bool(FUSE_BN_BWD_REDUCE_BF16 and not in_f32)      # (the sums select other kernels, never another launch plan)
    fams = ('conv_bf16_fwd', 'conv_bf16_dgrad', 'conv_bf16_wgrad') if ok else (None, None, None)
    return ConvPlanBF16(ok, *fams, one_launch, bn_fuse, bn_fuse, wgrad_bn, launches)


def _launches_bf16(descs, one_launch, out_f32):
    """cy_conv_gemm_bf16_plan's {BM, BN, TAPIN, ntiles, blocks} per launch (all descriptors in one, or one each); None if refused."""
    out = []
    for group in ([descs] if one_launch else [[d] for d in descs]):
        p = (C.c_int * 5)()
        if query('cy_conv_gemm_bf16_plan', (ConvGemm * len(group))(*group), len(group), 1 if out_f32 else 0, p) != 0:
            return None
        out.append(dict(BM=p[0], BN=p[1], TAPIN=p[2], ntiles=p[3], blocks=p[4]))
    return out


def conv_bf16_plans(op, in_shape, Cout, k, stride, pad, out_f32=False, bnf=False):
    """conv_plan_bf16(...).launches[op] by pass: op 'fwd' (in_shape = x's) or 'dgrad' (dx's); out_f32: that pass writes fp32.  bnf (the
    fused sums: input gradient with bf16 output only) selects other kernels, never another launch plan, so it is only checked."""
    got = None if bnf and (op == 'fwd' or out_f32) else conv_plan_bf16(in_shape, Cout, k, stride, pad, out_f32 and op == 'dgrad',
                                                                       out_f32 and op == 'fwd').launches[op]
    if not got:
        raise _lib.HipExtensionError('no bf16 %s launch for these shapes (bnf=%r): %s' % (op, bnf, query('capsyolo_last_error').decode()))
    return got


def _winograd(x, weight, bias, stats, transpose, f4, tag, out_slope=1.0):
    """x [B,H,W,Cg] NHWC; weight in PyTorch layout; transpose=True computes the input gradient of the layer; f4: on F(4x4,3x3).
    out_slope != 1: LeakyReLU epilogue (eval forward with the BatchNorm folded into weight / bias)."""
    B, H, W_, Cg = x.shape
    Cout_l, Cin_l = weight.shape[0], weight.shape[1]
    n = Cin_l if transpose else Cout_l
    st = _stream()
    u = _empty((query('cy_wino4_packed_floats' if f4 else 'cy_wino_packed_floats', Cg, n),), x)
    call('cy_wino4_pack_weights' if f4 else 'cy_wino_pack_weights', _ptr(weight), _ptr(u), Cout_l, Cin_l, 1 if transpose else 0, st)
    y = _empty((B, H, W_, n), x)
    # F(2x2,3x3) launches without an epilogue that fill at most half the chip (DarkNet's 13 x 13 input gradients) split their reduction
    nws = 0 if f4 else query('cy_wino_split_ws_floats', B, H, W_, Cg, n, int(bias is None and stats is None and out_slope == 1.0))
    ws = _empty((nws,), x) if nws > 0 else None
    with timer.range(('conv_wino4_' if f4 else 'conv_wino_') + ('dgrad/' if transpose else 'fwd/') + tag):
        if f4:
            call('cy_conv3x3_winograd4', _ptr(x), _ptr(u), _ptr(y), _ptr(bias), _ptr(stats), float(out_slope), B, H, W_, Cg, n, st)
        else:
            call('cy_conv3x3_winograd_ws', _ptr(x), _ptr(u), _ptr(y), _ptr(bias), _ptr(stats), float(out_slope), B, H, W_, Cg, n,
                 _ptr(ws), nws, st)
    return y


def conv1_affine_act(x, weight, bias, scale, shift, slope, tag='conv', out_bf16=False, mask=None):
    """lrelu((conv(x) + bias) * scale + shift) in one pass of the first-layer kernel (the second pass of its conv ->
    BatchNorm -> LeakyReLU block: recomputing the layer costs less than reading its 2.8 GB output back).
    out_bf16: the activation is written as bf16 (the bf16 path's second block reads it as such).
    mask: uint8 tensor of cy_conv1_signmask_bytes bytes that receives one bit per element, y > 0 (fp32 output only)."""
    B, _, Hi, Wi = x.shape
    Cout = weight.shape[0]
    with timer.range('conv1_fwd_act/' + tag):
        if mask is not None:
            if out_bf16:
                raise _lib.HipExtensionError('conv1_affine_act: the sign mask belongs to the fp32 activation pass')
            out = _empty((B, Hi, Wi, Cout), x)
            call('cy_conv1_3x3_fwd_act_mask', _ptr(x), _ptr(weight.contiguous()), _ptr(bias), _ptr(out), _ptr(scale), _ptr(shift),
                 float(slope), _ptr(mask), B, Hi, Wi, Cout, _stream())
        elif out_bf16:
            out = torch.empty((B, Hi, Wi, Cout), dtype=torch.bfloat16, device=x.device)
            call('cy_conv1_3x3_fwd_act_bf16', _ptr(x), _ptr(weight.contiguous()), _ptr(bias), _ptr(out), _ptr(scale), _ptr(shift),
                 float(slope), B, Hi, Wi, Cout, _stream())
        else:
            out = _empty((B, Hi, Wi, Cout), x)
            call('cy_conv1_3x3_fwd', _ptr(x), _ptr(weight.contiguous()), _ptr(bias), _ptr(out), None, _ptr(scale), _ptr(shift),
                 float(slope), B, Hi, Wi, Cout, _stream())
    return out


def conv_forward(x, weight, bias, k, stride, pad, nchw=False, stats=None, relu=False, tag='conv', in_affine=None, lrelu=None):
    """z[B,Ho,Wo,Cout] = conv2d(x) (+bias, optional fused ReLU); optional BN statistics side output.
    lrelu = slope in [0, 1]: LeakyReLU epilogue (the eval-mode forward of a block whose BatchNorm is folded into weight / bias)."""
    if lrelu is not None and (relu or stats is not None or in_affine is not None or not 0.0 <= lrelu <= 1.0):
        raise _lib.HipExtensionError('conv_forward: the LeakyReLU epilogue (slope %r) is the eval-mode forward: no statistics, no '
                                     'fused input affine, slope in [0, 1]' % (lrelu,))
    osl = 1.0 if lrelu is None else float(lrelu)
    x, weight = _f32(x, 'conv input'), _f32(weight, 'conv weight')
    B, Hi, Wi, Cin, xs = _x_geometry(x.shape, nchw)
    Cout = weight.shape[0]
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    plan = conv_plan(x.shape, Cout, k, stride, pad, nchw, relu, lrelu is not None)
    if in_affine is not None and not plan.in_affine:
        raise _lib.HipExtensionError('a fused input affine needs the 4x4/stride-2 Winograd kernels (got k=%d s=%d Cin=%d Cout=%d)' % (k, stride, Cin, Cout))
    if plan.fwd in ('conv_wino_fwd', 'conv_wino4_fwd'):
        return _winograd(x, weight, bias, stats, False, plan.fwd == 'conv_wino4_fwd', tag, osl)
    st = _stream()
    if plan.fwd in ('conv_wino2_fwd', 'conv_wino42_fwd'):
        pk, f4 = ('cy_wino4s2', '4') if plan.fwd == 'conv_wino42_fwd' else ('cy_wino2', '')
        y = _empty((B, Ho, Wo, Cout), x)
        isc, ish, isl = in_affine if in_affine is not None else (None, None, 1.0)
        u = _empty((query(pk + '_packed_floats', Cin, Cout),), x)
        call(pk + '_pack_weights', _ptr(weight), _ptr(u), Cout, Cin, st)
        with timer.range(plan.fwd + '/' + tag):
            call('cy_conv4x4s2_winograd' + f4, _ptr(x), _ptr(u), _ptr(y), _ptr(bias), _ptr(stats), _ptr(isc), _ptr(ish),
                 float(isl), osl, B, Hi, Wi, Cin, Cout, st)
        return y
    if plan.fwd == 'conv1_fwd':
        # the backbones' first layer (store-bound): persistent waves, operands from registers / L2
        z = _empty((B, Ho, Wo, Cout), x)
        with timer.range('conv1_fwd/' + tag):
            call('cy_conv1_3x3_fwd', _ptr(x), _ptr(weight.contiguous()), _ptr(bias), _ptr(z), _ptr(stats), None, None, 1.0,
                 B, Hi, Wi, Cout, st)
        return z
    wp = _empty((query('cy_conv_packed_floats', k * k * Cin, Cout),), x)
    call('cy_conv_pack_weights', _ptr(weight), _ptr(wp), Cout, Cin, k, k, k, k, 0, 0, 1, 0, st)
    z = _empty((B, Ho, Wo, Cout), x)
    a = _gemm_fwd_desc(B, Hi, Wi, Cin, xs, Cout, k, stride, pad, 1 if relu else 2 if lrelu is not None else 0, osl)
    a.X, a.Wp, a.Y = x.data_ptr(), wp.data_ptr(), z.data_ptr()
    a.bias, a.stats = bias.data_ptr() if bias is not None else None, stats.data_ptr() if stats is not None else None
    ws = _gemm_workspace(a, x)
    with timer.range('conv_gemm_fwd/' + tag):
        call('cy_conv_gemm', C.byref(a), st)
    del ws
    return z


def _gemm_workspace(a, like):
    """The optional workspace of one cy_conv_gemm launch (split reduction of under-filled grids, capsyolo_hip.h); the returned tensor
    must stay referenced until the call has been issued."""
    n = query('cy_conv_gemm_ws_floats', C.byref(a))
    if n <= 0:
        return None
    ws = _empty((n,), like)
    a.ws, a.ws_floats = ws.data_ptr(), n
    return ws


def dgrad_classes(Hi, Wi, k, stride, pad):
    """Input-gradient plan: one implicit GEMM per output-parity class (py, px) of the stride.

    Input pixel y = stride*oy' + py receives dz[oy' + dy0 - a] * W[kh0 + stride*a] for a in range(TH)
    (forward relation y = oy*stride - pad + kh).  Returns dicts with the cy_conv_gemm_t / cy_conv_pack_weights
    fields of each non-empty class; raises if some input pixel has no tap at all (kernel < stride)."""
    out = []
    for py in range(stride):
        kh0 = (py + pad) % stride
        TH = len(range(kh0, k, stride))
        for px in range(stride):
            kw0 = (px + pad) % stride
            TW = len(range(kw0, k, stride))
            Hv, Wv = (Hi - py + stride - 1) // stride, (Wi - px + stride - 1) // stride
            if Hv <= 0 or Wv <= 0:
                continue
            if TH == 0 or TW == 0:
                raise _lib.HipExtensionError('conv_dgrad: kernel %d / stride %d leaves input pixels without taps'
                                             % (k, stride))
            out.append(dict(TH=TH, TW=TW, kh0=kh0, kw0=kw0, kstep=stride, Ho=Hv, Wo=Wv,
                            dy0=(py + pad - kh0) // stride, dx0=(px + pad - kw0) // stride, dstep=-1,
                            out_stride=stride, out_oy=py, out_ox=px))
    return out


def _gemm_fwd_desc(B, Hi, Wi, Cin, xs, Cout, k, stride, pad, act=0, act_slope=1.0):
    """A forward's cy_conv_gemm_t without its pointers, fp32 or bf16 (xs: _x_geometry's strides; act 1: ReLU, 2: LeakyReLU)."""
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    return ConvGemm(xs_b=xs[0], xs_y=xs[1], xs_x=xs[2], xs_c=xs[3], B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo, N=Cout,
                    TH=k, TW=k, in_stride=stride, dy0=-pad, dx0=-pad, dstep=1, Hy=Ho, Wy=Wo, out_stride=1, out_oy=0, out_ox=0,
                    act=act, act_slope=act_slope)


def _gemm_dgrad_descs(in_shape, dz_shape, k, stride, pad):
    """An input gradient's parity classes (dgrad_classes) and their cy_conv_gemm_t without pointers, fp32 or bf16."""
    B, Hi, Wi, Cin = in_shape
    _, Ho, Wo, Cout = dz_shape
    classes = dgrad_classes(Hi, Wi, k, stride, pad)
    descs = (ConvGemm * len(classes))()
    for i, c in enumerate(classes):
        descs[i] = ConvGemm(xs_b=Ho * Wo * Cout, xs_y=Wo * Cout, xs_x=Cout, xs_c=1, B=B, Hi=Ho, Wi=Wo, Cin=Cout,
                            Ho=c['Ho'], Wo=c['Wo'], N=Cin, TH=c['TH'], TW=c['TW'], in_stride=1, dy0=c['dy0'], dx0=c['dx0'],
                            dstep=c['dstep'], Hy=Hi, Wy=Wi, out_stride=c['out_stride'], out_oy=c['out_oy'], out_ox=c['out_ox'], act=0)
    return classes, descs


def _set_bn_fuse(desc, bn_fuse):
    """The producer's BatchNorm (bn_fuse of conv_dgrad / conv_dgrad_bf16) into an input gradient's descriptor (cy_conv_gemm_t.bn_*)."""
    bz, bsc, bsh, bmu, bis, bsl, bred = bn_fuse
    desc.bn_z, desc.bn_scale, desc.bn_shift = bz.data_ptr(), bsc.data_ptr(), bsh.data_ptr()
    desc.bn_mean, desc.bn_invstd, desc.bn_red, desc.bn_slope = bmu.data_ptr(), bis.data_ptr(), bred.data_ptr(), float(bsl)


def conv_dgrad(dz, weight, in_shape, k, stride, pad, tag='conv', bn_fuse=None, plan=None):
    """dx[B,Hi,Wi,Cin] (NHWC) from dz[B,Ho,Wo,Cout]: one GEMM per output-parity class of the stride.
    bn_fuse = (z, scale, shift, mean, invstd, slope, red): dx is the gradient with respect to lrelu(z*scale+shift) of the
    producer block; the epilogues also accumulate that BatchNorm's backward sums into red[STATS_COPIES][Cin][2], and the 4x4 /
    stride-2 Winograd kernels then store dx * lrelu'(y), not dx (conv_plan(...).dgrad_premasks)."""
    dz, weight = _f32(dz, 'grad'), _f32(weight, 'conv weight')
    B, Hi, Wi, Cin = in_shape
    _, Ho, Wo, Cout = dz.shape
    plan = plan or conv_plan(in_shape, Cout, k, stride, pad)      # (a block's backward passes the one it asked for)
    if plan.dgrad in _WINO3_DGRAD:
        if bn_fuse is not None:
            raise _lib.HipExtensionError('bn_fuse is implemented in the direct input-gradient kernel only')
        return _winograd(dz, weight, None, None, True, plan.dgrad == 'conv_wino4_dgrad', tag)
    st = _stream()
    dx = _empty((B, Hi, Wi, Cin), dz)
    if plan.dgrad in ('conv_wino2_dgrad', 'conv_wino42_dgrad'):
        pk, f4 = ('cy_wino4s2', '4') if plan.dgrad == 'conv_wino42_dgrad' else ('cy_wino2', '')
        bz, bsc, bsh, bmu, bis, bsl, bred = bn_fuse if bn_fuse is not None else (None,) * 5 + (0.0, None)
        u = _empty((query(pk + '_dgrad_packed_floats', Cin, Cout),), dz)
        call(pk + '_pack_dgrad_weights', _ptr(weight), _ptr(u), Cout, Cin, st)
        with timer.range(plan.dgrad + '/' + tag):
            call('cy_conv4x4s2_winograd%s_dgrad' % f4, _ptr(dz), _ptr(u), _ptr(dx), _ptr(bz), _ptr(bsc), _ptr(bsh), _ptr(bmu),
                 _ptr(bis), float(bsl), _ptr(bred), B, Hi, Wi, Cin, Cout, st)
        return dx
    wp = _empty((query('cy_conv_packed_floats', ((k + stride - 1) // stride) ** 2 * Cout, Cin),), dz)
    for c, a in zip(*_gemm_dgrad_descs(in_shape, dz.shape, k, stride, pad)):
        call('cy_conv_pack_weights', _ptr(weight), _ptr(wp), Cout, Cin, k, k, c['TH'], c['TW'], c['kh0'], c['kw0'],
             c['kstep'], 1, st)
        a.X, a.Wp, a.Y = dz.data_ptr(), wp.data_ptr(), dx.data_ptr()
        if bn_fuse is not None:
            _set_bn_fuse(a, bn_fuse)
        ws = _gemm_workspace(a, dz)
        with timer.range('conv_gemm_dgrad/' + tag):
            call('cy_conv_gemm', C.byref(a), st)
        del ws
    return dx


def conv_wgrad(x, dz, k, stride, pad, nchw=False, tag='conv', in_affine=None, plan=None):
    x, dz = _f32(x, 'conv input'), _f32(dz, 'grad')
    B, Hi, Wi, Cin, xs = _x_geometry(x.shape, nchw)
    _, Ho, Wo, Cout = dz.shape
    st = _stream()
    dW = _empty((Cout, Cin, k, k), dz)
    plan = plan or conv_plan(x.shape, Cout, k, stride, pad, nchw)
    if in_affine is not None and not plan.in_affine:
        raise _lib.HipExtensionError('a fused input affine needs the 4x4/stride-2 Winograd weight-gradient kernel')
    if plan.wgrad == 'conv_wino4_wgrad':
        ws = _empty((query('cy_wino4_wgrad_ws_floats', B, Hi, Wi, Cin, Cout),), dz)
        with timer.range('conv_wino4_wgrad/' + tag):
            call('cy_conv3x3_winograd4_wgrad', _ptr(x), _ptr(dz), _ptr(dW), _ptr(ws), B, Hi, Wi, Cin, Cout, st)
    elif plan.wgrad == 'conv_wino_wgrad':
        ws = _empty((query('cy_wino_wgrad_ws_floats', B, Cin, Cout),), dz)
        with timer.range('conv_wino_wgrad/' + tag):
            call('cy_conv3x3_winograd_wgrad', _ptr(x), _ptr(dz), _ptr(dW), _ptr(ws), B, Hi, Wi, Cin, Cout, st)
    elif plan.wgrad == 'conv_wino2_wgrad':
        ws = _empty((query('cy_wino2_wgrad_ws_floats', B, Cin, Cout),), dz)
        isc, ish, isl = in_affine if in_affine is not None else (None, None, 1.0)
        with timer.range('conv_wino2_wgrad/' + tag):
            call('cy_conv4x4s2_winograd_wgrad', _ptr(x), _ptr(dz), _ptr(dW), _ptr(ws), _ptr(isc), _ptr(ish), float(isl),
                 B, Hi, Wi, Cin, Cout, st)
    elif plan.wgrad == 'conv1_wgrad':
        ws = _empty((query('cy_conv1_3x3_wgrad_ws_floats', B, Hi, Wi, Cout),), dz)
        with timer.range('conv1_wgrad/' + tag):
            call('cy_conv1_3x3_wgrad', _ptr(x), _ptr(dz), _ptr(dW), _ptr(ws), B, Hi, Wi, Cout, st)
    else:
        a = ConvWgrad(X=x.data_ptr(), dZ=dz.data_ptr(), dW=dW.data_ptr(), slabs=None,
                      xs_b=xs[0], xs_y=xs[1], xs_x=xs[2], xs_c=xs[3], B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo, N=Cout,
                      KH=k, KW=k, stride=stride, pad=pad)
        ws = _empty((query('cy_conv_wgrad_ws_floats', C.byref(a)),), dz)
        a.slabs = ws.data_ptr()
        with timer.range('conv_wgrad/' + tag):
            call('cy_conv_wgrad', C.byref(a), st)
    return dW


FOLD_EVAL_BN = True   # eval mode: the BatchNorm is folded into weights / bias once and the block's forward is conv + LeakyReLU epilogue
PARAM_EPOCH = 0       # bumped by everything that writes parameters / running statistics through raw pointers (optim.Adam.step,
                      # cy_bn_finalize in a training forward): part of the fold cache's key next to the tensors' version counters


def _bump_param_epoch():
    global PARAM_EPOCH
    PARAM_EPOCH += 1


def fold_eval_bn(weight, bias, gamma, beta, bn):
    """(W', b') of the eval-mode block: W'[co] = W[co] * s[co], b' = (b - running_mean) * s + beta, s = gamma / sqrt(running_var
    + eps) (cy_bn_fold_eval), cached on the BatchNorm module until a parameter or running statistic changes."""
    ts = (weight, bias, gamma, beta, bn.running_mean, bn.running_var)
    key = (PARAM_EPOCH, float(bn.eps)) + tuple((t.data_ptr(), t._version) if t is not None else None for t in ts)
    hit = getattr(bn, '_cy_fold', None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    weight = _f32(weight, 'conv weight')
    Wf, bf = torch.empty_like(weight), _empty((weight.shape[0],), weight)
    call('cy_bn_fold_eval', _ptr(weight), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(bn.running_mean), _ptr(bn.running_var),
         float(bn.eps), _ptr(Wf), _ptr(bf), weight.shape[0], weight.numel() // weight.shape[0], _stream())
    bn._cy_fold = (key, Wf, bf)
    return Wf, bf


class ConvBlockCfg(object):
    """Static description of one conv (+BatchNorm) (+activation) block: no forward or backward writes to it, so one cfg may
    serve any number of steps.  What travels between two blocks of one step is a BnHandover, not an attribute here."""

    def __init__(self, k, stride, pad, nchw_in=False, bn=None, slope=None, name='conv', defer_act=False):
        self.k, self.stride, self.pad, self.nchw_in, self.name = k, stride, pad, nchw_in, name
        self.defer_act = defer_act   # return (z, BnHandover): the consumer applies BatchNorm + LeakyReLU on its loads
        self.out_bf16 = False        # fp32 first block of the bf16 backbone: the activation leaves as bf16, the gradient arrives as bf16
        self.in_f32 = self.out_f32 = False   # bf16 block: x comes from an fp32 producer / the activation leaves for an fp32 consumer
        self.bn = bn            # module with running_mean / running_var / momentum / eps / training, or None
        self.slope = slope      # None: no activation; 0.0: ReLU; else LeakyReLU slope


class BnHandover(object):
    """What a conv -> BatchNorm -> LeakyReLU block (the PRODUCER) hands to the block that reads its output (the CONSUMER).
    scale / shift / slope let the consumer of a raw output z apply the activation on its loads; mean / invstd (None in eval
    mode) and, on the bf16 path, z let its input-gradient kernel also sum the producer's BatchNorm backward.  The consumer's
    backward GIVES those sums: give_red(red [C][2] double, premasked = its gradient already carries the activation's
    derivative).  The producer's backward, which runs afterwards, TAKES them exactly once: take_red() -> (red, premasked),
    or None when nobody gave any (it then sums for itself); after a take the object is empty again."""
    __slots__ = ('z', 'scale', 'shift', 'mean', 'invstd', 'slope', '_red')

    def __init__(self, scale, shift, mean, invstd, slope, z=None):
        self.z, self.scale, self.shift, self.mean, self.invstd, self.slope = z, scale, shift, mean, invstd, float(slope)
        self._red = None

    def give_red(self, red, premasked):
        self._red = (red, bool(premasked))

    def take_red(self):
        got, self._red = self._red, None
        return got


SYNC_BN = False     # data parallel only: BatchNorm statistics (forward sums, backward sums) summed over all ranks, so
                    # that N ranks x batch B train exactly like one process on the global batch N*B


def _sync_world():
    import torch.distributed as dist
    if SYNC_BN and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist, dist.get_world_size()
    return None, 1


def _bn_finalize(stats, P, gamma, beta, bn, scale, shift, mean, invstd, N, st):
    """Batch statistics (summed over all ranks under SYNC_BN) -> scale / shift / mean / invstd and the running statistics."""
    dist, world = _sync_world()
    if dist is not None:              # sum z / sum z^2 over the global batch (equal shards: dp.shard_range)
        dist.all_reduce(stats)
    call('cy_bn_finalize', _ptr(stats), P * world, _ptr(gamma), _ptr(beta), _ptr(bn.running_mean),
         _ptr(bn.running_var), float(bn.momentum), float(bn.eps), _ptr(scale), _ptr(shift), _ptr(mean),
         _ptr(invstd), N, _ptr(bn.num_batches_tracked), st)
    _bump_param_epoch()               # running statistics were written through raw pointers


def _leave(out, cfg, st):
    """The fp32 activation on its way out: as bf16 where the consumer is a bf16 block (FusedBackbone._forward_bf16)."""
    if not cfg.out_bf16:
        return out
    ob = torch.empty(out.shape, dtype=torch.bfloat16, device=out.device)
    call('cy_cast_f32_bf16', _ptr(out), _ptr(ob), out.numel(), st)
    return ob


def _sync_red(red, N, st):
    """The BatchNorm-backward sums red [N][2] of this rank -> of the global batch (data parallel under SYNC_BN; else as they are)."""
    dist, world = _sync_world()
    if dist is not None:
        # global sums / world: the apply kernel divides by the LOCAL pixel count, which then gives the global
        # means; dgamma / dbeta come out as (global sum) / world, what the gradient all-reduce MEAN expects
        red = red.contiguous()
        call('cy_bn_red_fold', _ptr(red), 1, 1.0 / world, _ptr(red), None, None, N, st)    # in place: sum of the pre-scaled = mean
        dist.all_reduce(red)
    return red


def _grad_f32(da, cfg, keep_bf16=False):
    """The gradient that reached a block's output, as fp32 (keep_bf16: only the first-layer kernels read a bf16 gradient)."""
    if da is None:
        raise _lib.HipExtensionError('conv block %s: no gradient reached its output' % cfg.name)
    if da.dtype == torch.bfloat16 and cfg.out_bf16:
        if keep_bf16:
            return da.contiguous()
        daf = torch.empty(da.shape, dtype=torch.float32, device=da.device)
        call('cy_cast_bf16_f32', _ptr(da.contiguous()), _ptr(daf), da.numel(), _stream())
        return daf
    return _f32(da, 'grad')


def _input_grad(ctx, dz, x, weight, plan, st):
    """dx of a block whose input wants one (plan: a ConvPlan or a ConvPlanBF16); as the CONSUMER of ctx.hin, the input-gradient
    kernel's epilogue also sums the producer's BatchNorm backward where the plan has that form, and the sums are given to the
    hand-over.  The producer's z is x itself on the fp32 path (mean / invstd only in training mode); a bf16 producer hands its z over."""
    if not ctx.needs_input_grad[0]:
        return None
    bf16 = isinstance(plan, ConvPlanBF16)
    cfg, h, fuse = ctx.cfg, ctx.hin, None
    if plan.dgrad is None and not bf16:
        if cfg.nchw_in and image_grad_plan(x.shape, weight.shape[0], cfg.k, cfg.stride, cfg.pad).ok:
            return conv_image_grad(dz, weight, tuple(x.shape), cfg.k, cfg.pad, tag=cfg.name)     # a first layer: the gradient of the image
        raise _lib.HipExtensionError('input gradient of an NCHW-input convolution is not implemented')
    if plan.dgrad_bn_fuse and h is not None and (tuple(h.z.shape) == tuple(x.shape) if bf16 else h.mean is not None):
        bred = zero_pool.take((STATS_COPIES, x.shape[3], 2), torch.float64, x.device)
        fuse = (h.z if bf16 else x, h.scale, h.shift, h.mean, h.invstd, h.slope, bred)
    if bf16:
        dx = conv_dgrad_bf16(dz, weight, tuple(x.shape), cfg.k, cfg.stride, cfg.pad, cfg.in_f32, cfg.name, fuse, plan)
    else:
        dx = conv_dgrad(dz, weight, tuple(x.shape), cfg.k, cfg.stride, cfg.pad, cfg.name, fuse, plan)
    if fuse is not None:
        red = _empty((x.shape[3], 2), x, torch.float64)
        call('cy_bn_red_fold', _ptr(bred), STATS_COPIES, 1.0, _ptr(red), None, None, x.shape[3], st)
        h.give_red(red, plan.dgrad_premasks)
    return dx


class _ConvBlockNoBn(torch.autograd.Function):
    """conv -> [[Leaky]ReLU], saving x and z."""

    @staticmethod
    def forward(ctx, x, weight, bias, cfg, hin):
        x, weight = _f32(x, 'conv input'), _f32(weight, 'conv weight')
        if cfg.defer_act:
            raise _lib.HipExtensionError('defer_act needs a BatchNorm block')
        N = weight.shape[0]
        ctx.cfg, ctx.has_bias, ctx.hin = cfg, bias is not None, hin
        ctx.in_affine = None if hin is None else (hin.scale, hin.shift, hin.slope)      # x is the raw output of a deferring producer
        ctx.set_materialize_grads(False)
        relu = cfg.slope is not None and cfg.slope == 0.0
        z = conv_forward(x, weight, bias, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in, None, relu, cfg.name, ctx.in_affine)
        out = z
        if cfg.slope is not None and not relu:
            out = torch.empty_like(z)
            call('cy_affine_act', _ptr(z), _ptr(out), None, None, float(cfg.slope), z.numel() // N, N, _stream())
        ctx.save_for_backward(x, weight, z)
        return out

    @staticmethod
    def backward(ctx, da):
        cfg = ctx.cfg
        dz = da = _grad_f32(da, cfg)
        st = _stream()
        x, weight, z = ctx.saved_tensors
        N = weight.shape[0]
        plan = conv_plan(x.shape, N, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        # a first layer with an activation: the image-gradient kernel takes the activation's derivative from the sign of z on its
        # loads of da (z and the block's output have one sign for a slope in [0, 1]), so dx needs no dz in memory
        image = bool(need_x and cfg.nchw_in and cfg.slope is not None and 0.0 <= float(cfg.slope) <= 1.0
                     and image_grad_plan(x.shape, N, cfg.k, cfg.stride, cfg.pad).ok)
        if cfg.slope is not None and (need_w or need_b or (need_x and not image)):
            dz = torch.empty_like(z)
            call('cy_act_bwd', _ptr(z), _ptr(da), _ptr(dz), float(cfg.slope), z.numel(), st)
        dbias = channel_sum(dz, N, st) if need_b else None
        dW = conv_wgrad(x, dz, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in, cfg.name, ctx.in_affine, plan) if need_w else None
        if image:
            return conv_image_grad(da, weight, tuple(x.shape), cfg.k, cfg.pad, z, float(cfg.slope), None, cfg.name), dW, dbias, None, None
        return _input_grad(ctx, dz, x, weight, plan, st), dW, dbias, None, None


def channel_sum(dz, N, st=None):
    """out[n] = sum over the rows of dz [P, N] (the bias gradient of a convolution without BatchNorm) in a fixed order: with more than one
    row split through cy_channel_sum_ws and its partials, so that the same dz gives the same bits in every run (cy_channel_sum adds its
    splits with float atomics); with one split cy_channel_sum is a fixed order already."""
    st = _stream() if st is None else st
    P = dz.numel() // N
    out = _empty((N,), dz)
    need = query('cy_channel_sum_ws_floats', P, N)
    if need:
        ws = _empty((need,), dz)
        call('cy_channel_sum_ws', _ptr(dz), _ptr(out), _ptr(ws), need, P, N, st)
    else:
        call('cy_channel_sum', _ptr(dz), _ptr(out), P, N, st)
    return out


class _Conv1TrainBlock(torch.autograd.Function):
    """The first block (3 -> {32, 64, 128} channels, NCHW image; csrc/conv1.hip) in training mode: conv -> BatchNorm ->
    LeakyReLU without z in memory.  The forward takes the statistics (from the moment matrix of the input patches, or from one
    pass that computes the layer and keeps nothing) and then writes the activation; the backward passes recompute the
    convolution and read only the gradient.  The image gets no gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, cfg, plan):
        x, weight = _f32(x, 'conv input'), _f32(weight, 'conv weight')
        st = _stream()
        N = weight.shape[0]
        Bx, _, Hx, Wx = x.shape
        ctx.cfg, ctx.has_bias, ctx.m2, ctx.mask = cfg, bias is not None, None, None
        ctx.set_materialize_grads(False)
        scale, shift, mean, invstd = (_empty((N,), x) for _ in range(4))
        stats = zero_pool.take((STATS_COPIES, N, 2), torch.float64, x.device)
        if plan.conv1_moments:
            # sum z and sum z^2 from the moment matrix of the input patches: the layer is not computed for them
            wsm = _empty((query('cy_conv1_3x3_stats_ws_floats', Bx, Hx),), x)
            with timer.range('conv1_fwd_stats/' + cfg.name):
                call('cy_conv1_3x3_stats', _ptr(x), _ptr(weight.contiguous()), _ptr(bias), _ptr(stats), _ptr(wsm),
                     Bx, Hx, Wx, N, st)
            off = query('cy_conv1_3x3_stats_m2_offset', Bx, Hx)
            ctx.m2 = wsm[off:off + 2048]    # the double M2[32][32]: the one-pass backward reads it
        else:
            with timer.range('conv1_fwd_stats/' + cfg.name):
                call('cy_conv1_3x3_fwd', _ptr(x), _ptr(weight.contiguous()), _ptr(bias), None, _ptr(stats), None, None,
                     1.0, Bx, Hx, Wx, N, st)
        _bn_finalize(stats, Bx * Hx * Wx, gamma, beta, cfg.bn, scale, shift, mean, invstd, N, st)
        if plan.conv1_signmask and ctx.m2 is not None and not cfg.out_bf16 and _sync_world()[0] is None:
            # the fp32 block: the one-pass backward will want the sign of y and nothing else of z
            ctx.mask = torch.empty((query('cy_conv1_signmask_bytes', Bx, Hx, Wx, N),), dtype=torch.uint8, device=x.device)
        ctx.save_for_backward(x, weight, bias, scale, shift, mean, invstd)
        slope = 1.0 if cfg.slope is None else float(cfg.slope)
        return conv1_affine_act(x, weight, bias, scale, shift, slope, cfg.name, cfg.out_bf16, ctx.mask)

    @staticmethod
    def backward(ctx, da):
        cfg = ctx.cfg
        da = _grad_f32(da, cfg, keep_bf16=True)
        da_bf16 = da.dtype == torch.bfloat16
        st = _stream()
        x, weight, bias, scale, shift, mean, invstd = ctx.saved_tensors
        N, slope = weight.shape[0], 1.0 if cfg.slope is None else float(cfg.slope)
        B, _, Hi, Wi = x.shape
        plan = conv_plan(x.shape, N, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in)
        # both passes recompute z tile by tile and read only da; dz is formed in registers in the layout the weight-gradient
        # MFMA consumes (csrc/conv1.hip)
        redc = zero_pool.take((STATS_COPIES, N, 2), torch.float64, x.device)
        dW, dbeta, dgamma = _empty(tuple(weight.shape), x), _empty((N,), x), _empty((N,), x)
        ws = _empty((query('cy_conv1_bn_bwd_wgrad_ws_floats', B, Hi, Wi, N),), x)
        common = (_ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd), slope)
        if plan.conv1_onepass and ctx.m2 is not None and _sync_world()[0] is None:
            # one pass over da: sum d and the weight gradient OF d; the rest follows from the forward's patch moments
            tail = (_ptr(ctx.m2), _ptr(redc), _ptr(dW), _ptr(dgamma), _ptr(dbeta), None, _ptr(ws), B, Hi, Wi, N, st)
            with timer.range('conv1_bn_bwd_onepass/' + cfg.name):
                if ctx.mask is not None and not da_bf16 and da.data_ptr() % 16 == 0:
                    call('cy_conv1_bn_bwd_onepass_mask', _ptr(x), _ptr(weight), _ptr(bias), _ptr(da), _ptr(ctx.mask), *(common + tail))
                else:
                    call('cy_conv1_bn_bwd_onepass_bf16' if da_bf16 else 'cy_conv1_bn_bwd_onepass', _ptr(x), _ptr(weight),
                         _ptr(bias), _ptr(da), *(common + tail))
        else:
            with timer.range('conv1_bn_bwd_reduce/' + cfg.name):
                call('cy_conv1_bn_bwd_reduce_bf16' if da_bf16 else 'cy_conv1_bn_bwd_reduce', _ptr(x), _ptr(weight), _ptr(bias),
                     _ptr(da), *(common + (_ptr(redc), B, Hi, Wi, N, st)))
            red = _empty((N, 2), x, torch.float64)
            dist, world = _sync_world()
            # copies folded (and, data parallel, pre-scaled by 1 / world so that the all-reduce SUM is the mean)
            call('cy_bn_red_fold', _ptr(redc), STATS_COPIES, 1.0 / world, _ptr(red), _ptr(dgamma), _ptr(dbeta), N, st)
            if dist is not None:
                dist.all_reduce(red)
                call('cy_bn_red_fold', _ptr(red), 1, 1.0, None, _ptr(dgamma), _ptr(dbeta), N, st)
            with timer.range('conv1_bn_bwd_wgrad/' + cfg.name):
                call('cy_conv1_bn_bwd_wgrad_bf16' if da_bf16 else 'cy_conv1_bn_bwd_wgrad', _ptr(x), _ptr(weight), _ptr(bias),
                     _ptr(da), *(common + (_ptr(red), B * Hi * Wi, _ptr(dW), _ptr(ws), B, Hi, Wi, N, st)))
        dbias = _const_zeros(N, x) if ctx.has_bias else None     # in front of BatchNorm: analytically zero
        return None, dW, dbias, dgamma, dbeta, None, None


class _ConvBnBlock(torch.autograd.Function):
    """conv -> BatchNorm (batch statistics from the conv epilogue) -> [Leaky]ReLU, saving only x and z: every BatchNorm block
    that is not the first layer's training block.  hin: the hand-over of a producer whose raw output x is (the BatchNorm +
    LeakyReLU of that block are applied on this block's loads).  cfg.defer_act: returns (z, BnHandover) and leaves the
    activation to the consumer.  Eval mode runs on the running statistics -- folded into weights / bias where that is one
    launch -- and its backward gives the input gradient alone, on the folded path, when the input asked for one (eval_dx)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, cfg, plan, hin, eval_dx=False):
        x, weight = _f32(x, 'conv input'), _f32(weight, 'conv weight')
        st = _stream()
        N = weight.shape[0]
        bn = cfg.bn
        ctx.cfg, ctx.has_bias, ctx.bn_train, ctx.hin, ctx.hout = cfg, bias is not None, bool(bn.training), hin, None
        ctx.eval_dx, ctx.x_shape = False, tuple(x.shape)
        ctx.set_materialize_grads(False)      # the hand-over that leaves next to z is no tensor and gets no gradient
        ctx.in_affine = ina = None if hin is None else (hin.scale, hin.shift, hin.slope)
        scale, shift, mean, invstd = (_empty((N,), x) for _ in range(4))
        slope = 1.0 if cfg.slope is None else float(cfg.slope)
        if bn.training:
            stats = zero_pool.take((STATS_COPIES, N, 2), torch.float64, x.device)
            z = conv_forward(x, weight, bias, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in, stats, False, cfg.name, ina)
            _bn_finalize(stats, z.numel() // N, gamma, beta, bn, scale, shift, mean, invstd, N, st)
        else:
            if FOLD_EVAL_BN and not cfg.defer_act and ina is None and 0.0 <= slope <= 1.0:
                # eval mode (predict_fns.py:38-43, 65-69): ONE launch per block.  The first layer applies scale / shift in its
                # own epilogue (its kernel takes them); every other layer runs on weights and bias with the BatchNorm folded in
                # eval_dx (conv_block: the input wants a gradient): what the input gradient needs is kept -- the output for the
                # sign of z, and the weight the forward ran on (a first-layer block: the raw weight and the BatchNorm scale)
                ctx.eval_dx = bool(eval_dx and not cfg.out_bf16)
                if plan.conv1:
                    call('cy_bn_eval_scale_shift', _ptr(gamma), _ptr(beta), _ptr(bn.running_mean), _ptr(bn.running_var),
                         float(bn.eps), _ptr(scale), _ptr(shift), N, st)
                    out = conv1_affine_act(x, weight, bias, scale, shift, slope, cfg.name, cfg.out_bf16)
                    ctx.save_for_backward(*((out, weight, scale) if ctx.eval_dx else ()))
                    return out
                Wf, bf = fold_eval_bn(weight, bias, gamma, beta, bn)
                out = conv_forward(x, Wf, bf, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in, None, False, cfg.name, None, lrelu=slope)
                ctx.save_for_backward(*((out, Wf, None) if ctx.eval_dx else ()))
                return _leave(out, cfg, st)
            z = conv_forward(x, weight, bias, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in, None, False, cfg.name, ina)
            call('cy_bn_eval_scale_shift', _ptr(gamma), _ptr(beta), _ptr(bn.running_mean), _ptr(bn.running_var),
                 float(bn.eps), _ptr(scale), _ptr(shift), N, st)
        ctx.save_for_backward(x, weight, z, scale, shift, mean, invstd, gamma)
        if cfg.defer_act:
            # the consumer applies lrelu(z * scale + shift) on its loads; in training mode its input-gradient kernel can also
            # sum this block's BatchNorm backward, for which it needs mean / invstd
            ctx.hout = BnHandover(scale, shift, mean if ctx.bn_train else None, invstd if ctx.bn_train else None, slope)
            return z, ctx.hout
        if plan.conv1 and 0.0 <= slope <= 1.0:
            return conv1_affine_act(x, weight, bias, scale, shift, slope, cfg.name, cfg.out_bf16)
        out = torch.empty_like(z)
        call('cy_affine_act', _ptr(z), _ptr(out), _ptr(scale), _ptr(shift), slope, z.numel() // N, N, st)
        return _leave(out, cfg, st)

    @staticmethod
    def backward(ctx, da, _hout=None):
        cfg = ctx.cfg
        da = _grad_f32(da, cfg)
        if not ctx.bn_train:
            if not ctx.eval_dx:
                raise _lib.HipExtensionError('backward through an eval-mode BatchNorm block is not implemented')
            return (_ConvBnBlock._eval_input_grad(ctx, da),) + (None,) * 8
        st = _stream()
        x, weight, z, scale, shift, mean, invstd, gamma = ctx.saved_tensors
        N = weight.shape[0]
        P = z.numel() // N
        plan = conv_plan(x.shape, N, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in)
        slope = 1.0 if cfg.slope is None else float(cfg.slope)
        given = ctx.hout.take_red() if ctx.hout is not None else None
        if given is not None:
            # summed by the consumer block's input-gradient epilogues, whose stride-2 Winograd kernel (and the fused max-pool
            # backward) has then also applied the activation's derivative to da already
            red, premasked = given
            if premasked:
                slope = 1.0
        else:
            red, premasked = _empty((N, 2), z, torch.float64), False
            call('cy_bn_bwd_reduce', _ptr(z), _ptr(da), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd), slope,
                 _ptr(red), P, N, st)
        red = _sync_red(red, N, st)
        dz = torch.empty_like(z)
        dgamma, dbeta = _empty((N,), z), _empty((N,), z)
        # a bias in front of BatchNorm has an analytically zero gradient: sum(dz) == 0
        dbias = _const_zeros(N, z) if ctx.has_bias else None
        if plan.wgrad_bn and ctx.hin is None:
            # pass 2 of the BatchNorm backward inside the Winograd weight-gradient kernel, which has every dz element in
            # registers on its way to LDS anyway and writes it out for the input-gradient kernel
            red = red.contiguous()
            call('cy_bn_param_grad', _ptr(red), _ptr(dgamma), _ptr(dbeta), N, st)
            B_, Hi, Wi, Cin = x.shape
            dW = _empty(tuple(weight.shape), z)
            if premasked and plan.wgrad_bn4:
                ws = _empty((query('cy_wino4_wgrad_ws_floats', B_, Hi, Wi, Cin, N),), z)
                with timer.range('conv_wino4_wgrad_bn/' + cfg.name):
                    call('cy_conv3x3_winograd4_wgrad_bn', _ptr(x), _ptr(z), _ptr(da), _ptr(dz), _ptr(scale),
                         _ptr(mean), _ptr(invstd), _ptr(red), P, _ptr(dW), _ptr(ws), B_, Hi, Wi, Cin, N, st)
            else:
                ws = _empty((query('cy_wino_wgrad_ws_floats', B_, Cin, N),), z)
                with timer.range('conv_wino_wgrad_bn/' + cfg.name):
                    call('cy_conv3x3_winograd_wgrad_bn', _ptr(x), _ptr(z), _ptr(da), _ptr(dz), _ptr(scale),
                         _ptr(shift), _ptr(mean), _ptr(invstd), slope, 1 if premasked else 0, _ptr(red), P, _ptr(dW), _ptr(ws),
                         B_, Hi, Wi, Cin, N, st)
        else:
            call('cy_bn_bwd_apply', _ptr(z), _ptr(da), _ptr(dz), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd),
                 _ptr(gamma), slope, _ptr(red), _ptr(dgamma), _ptr(dbeta), P, N, st)
            dW = conv_wgrad(x, dz, cfg.k, cfg.stride, cfg.pad, cfg.nchw_in, cfg.name, ctx.in_affine, plan)
        return _input_grad(ctx, dz, x, weight, plan, st), dW, dbias, dgamma, dbeta, None, None, None, None

    @staticmethod
    def _eval_input_grad(ctx, da):
        """dx of a folded eval-mode block, and nothing else: lrelu'(z) from the sign of the saved output, the BatchNorm scale inside
        the weight the forward ran on (or, for a first-layer block, on the image-gradient kernel's loads)."""
        cfg = ctx.cfg
        if any(ctx.needs_input_grad[1:5]):
            raise _lib.HipExtensionError('conv block %s: an eval-mode BatchNorm block gives the input gradient only; its weight, bias, '
                                         'gamma and beta get no gradient there (switch their requires_grad off, or train())' % cfg.name)
        out, weight, scale = ctx.saved_tensors
        slope = 1.0 if cfg.slope is None else float(cfg.slope)
        if cfg.nchw_in:
            if not image_grad_plan(ctx.x_shape, weight.shape[0], cfg.k, cfg.stride, cfg.pad).ok:
                raise _lib.HipExtensionError('input gradient of an NCHW-input convolution is not implemented')
            return conv_image_grad(da, weight, ctx.x_shape, cfg.k, cfg.pad, out, slope, scale, cfg.name)
        dz = da
        if slope != 1.0:
            dz = torch.empty_like(out)
            call('cy_act_bwd', _ptr(out), _ptr(da), _ptr(dz), slope, out.numel(), _stream())
        return conv_dgrad(dz, weight, ctx.x_shape, cfg.k, cfg.stride, cfg.pad, cfg.name)


# ------------------------------------------------------------------------------------------------ bf16 convolution path
def _bf(t, name='tensor'):
    if not (t.is_cuda and t.dtype == torch.bfloat16):
        raise _lib.HipExtensionError('%s must be a bfloat16 tensor on the GPU (got %s on %s)' % (name, t.dtype, t.device))
    return t if t.is_contiguous() else t.contiguous()


def cast_bf16(x):
    """fp32 -> bf16 (round to nearest even); the gradient passes through unchanged (it arrives in fp32)."""
    return _CastBF16.apply(x)


class _CastBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        call('cy_cast_f32_bf16', _ptr(x), _ptr(y), x.numel(), _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy.dtype == torch.bfloat16:
            out = torch.empty(dy.shape, dtype=torch.float32, device=dy.device)
            call('cy_cast_bf16_f32', _ptr(_bf(dy)), _ptr(out), dy.numel(), _stream())
            return out
        return dy


def conv_forward_bf16(x, weight, bias, k, stride, pad, stats=None, tag='conv', lrelu=None, out_f32=False):
    """z (bf16 NHWC) = conv2d(x bf16 NHWC) + bias with fp32 accumulation; optional BatchNorm statistics.
    lrelu = slope in [0, 1]: LeakyReLU epilogue (eval forward, BatchNorm folded into weight / bias); out_f32: fp32 output."""
    x, weight = _bf(x, 'conv input'), _f32(weight, 'conv weight')
    B, Hi, Wi, Cin, xs = _x_geometry(x.shape, False)
    Cout = weight.shape[0]
    st = _stream()
    wp = torch.empty((query('cy_conv_bf16_packed_elems', k * k * Cin, Cout),), dtype=torch.bfloat16, device=x.device)
    call('cy_conv_bf16_pack_weights', _ptr(weight), _ptr(wp), Cout, Cin, k, k, k, k, 0, 0, 1, 0, st)
    a = _gemm_fwd_desc(B, Hi, Wi, Cin, xs, Cout, k, stride, pad, 0 if lrelu is None else 2, 1.0 if lrelu is None else float(lrelu))
    z = torch.empty((B, a.Ho, a.Wo, Cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    a.X, a.Wp, a.Y = x.data_ptr(), wp.data_ptr(), z.data_ptr()
    a.bias, a.stats = bias.data_ptr() if bias is not None else None, stats.data_ptr() if stats is not None else None
    with timer.range('conv_bf16_fwd/' + tag):
        call('cy_conv_gemm_bf16', C.byref(a), 1 if out_f32 else 0, st)
    return z


def conv_dgrad_bf16(dz, weight, in_shape, k, stride, pad, out_f32=False, tag='conv', bn_fuse=None, plan=None):
    """dx [B,Hi,Wi,Cin] (bf16, or fp32 for an fp32 producer) from dz (bf16): one GEMM per output-parity class.
    bn_fuse = (z bf16, scale, shift, mean, invstd, slope, red[STATS_COPIES][Cin][2]) of the PRODUCER block (bf16 output only): the
    epilogues store d = dx * lrelu'(z * scale + shift) -- the premasked gradient -- and add sum d, sum d * xhat of the stored
    (bf16-rounded) values to red, all parity classes together (cy_conv_gemm_t.bn_*)."""
    dz, weight = _bf(dz, 'grad'), _f32(weight, 'conv weight')
    if bn_fuse is not None and out_f32:
        raise _lib.HipExtensionError('conv_dgrad_bf16: the fused BatchNorm-backward sums are built for the bf16 output')
    B, Hi, Wi, Cin = in_shape
    Cout = dz.shape[3]
    plan = plan or conv_plan_bf16(in_shape, Cout, k, stride, pad, in_f32=out_f32)      # (a block's backward passes the one it asked for)
    st = _stream()
    dx = torch.empty((B, Hi, Wi, Cin), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dz.device)
    classes, descs = _gemm_dgrad_descs(in_shape, dz.shape, k, stride, pad)
    nel = query('cy_conv_bf16_packed_elems', ((k + stride - 1) // stride) ** 2 * Cout, Cin)
    wp = torch.empty((len(classes), nel), dtype=torch.bfloat16, device=dz.device)
    for i, c in enumerate(classes):
        call('cy_conv_bf16_pack_weights', _ptr(weight), _ptr(wp[i]), Cout, Cin, k, k, c['TH'], c['TW'], c['kh0'], c['kw0'],
             c['kstep'], 1, st)
        a = descs[i]
        a.X, a.Wp, a.Y = dz.data_ptr(), wp[i].data_ptr(), dx.data_ptr()
        if bn_fuse is not None:
            _set_bn_fuse(a, (_bf(bn_fuse[0], 'producer z'),) + tuple(bn_fuse[1:]))
    if plan.dgrad_one_launch:
        with timer.range('conv_bf16_dgrad/' + tag):
            call('cy_conv_gemm_bf16_classes', descs, len(classes), 1 if out_f32 else 0, st)
    else:
        for i in range(len(classes)):
            with timer.range('conv_bf16_dgrad/' + tag):
                call('cy_conv_gemm_bf16', C.byref(descs[i]), 1 if out_f32 else 0, st)
    return dx


def conv_wgrad_bf16(x, dz, k, stride, pad, tag='conv'):
    x, dz = _bf(x, 'conv input'), _bf(dz, 'grad')
    B, Hi, Wi, Cin = x.shape
    _, Ho, Wo, Cout = dz.shape
    nws = query('cy_conv_wgrad_bf16_ws_floats', B, Ho, Wo, Cin, Cout, k, stride)
    if nws < 0 or pad != 1:
        raise _lib.HipExtensionError('bf16 weight gradient: unsupported layer k=%d s=%d p=%d Cin=%d Cout=%d' % (k, stride, pad, Cin, Cout))
    ws = _empty((nws,), dz)
    dW = _empty((Cout, Cin, k, k), dz)
    with timer.range('conv_bf16_wgrad/' + tag):
        call('cy_conv_wgrad_bf16', _ptr(x), _ptr(dz), _ptr(dW), _ptr(ws), B, Hi, Wi, Cin, Ho, Wo, Cout, k, stride, _stream())
    return dW


class _ConvBlockBF16(torch.autograd.Function):
    """conv -> BatchNorm (batch statistics from the conv epilogue) -> LeakyReLU on the bf16 kernels: x, the raw conv output
    z and the activation are bf16 NHWC; statistics, scale / shift and all parameter gradients are fp32 / double.
    cfg.out_f32: the activation leaves in fp32 (its consumer is an fp32 kernel: the routing head); cfg.in_f32: x was
    cast from an fp32 producer, whose backward wants its gradient in fp32.  hin: the BnHandover of the bf16 block in front, or
    None.  Returns (activation, this block's BnHandover for its consumer -- None where the consumer cannot sum for it)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, cfg, hin):
        st = _stream()
        if cfg.in_f32:
            # the producer is an fp32 kernel (the first block): round its activation to bf16 HERE, so that autograd sees an
            # fp32 input and takes the fp32 gradient this block's input-gradient kernel writes (a separate cast Function made
            # the engine convert that gradient to bf16 and back: two 3 GB passes at 608 x 608)
            xf = _f32(x, 'conv input')
            x = torch.empty(xf.shape, dtype=torch.bfloat16, device=xf.device)
            call('cy_cast_f32_bf16', _ptr(xf), _ptr(x), xf.numel(), st)
        x, weight = _bf(x, 'conv input'), _f32(weight, 'conv weight')
        N = weight.shape[0]
        bn = cfg.bn
        if bn is None or cfg.slope is None:
            raise _lib.HipExtensionError('the bf16 path is built for conv -> BatchNorm -> LeakyReLU blocks')
        ctx.cfg, ctx.has_bias, ctx.bn_train, ctx.hin, ctx.hout = cfg, bias is not None, bool(bn.training), hin, None
        scale, shift, mean, invstd = (_empty((N,), weight) for _ in range(4))
        if bn.training:
            stats = zero_pool.take((STATS_COPIES, N, 2), torch.float64, x.device)
            z = conv_forward_bf16(x, weight, bias, cfg.k, cfg.stride, cfg.pad, stats, cfg.name)
            P = z.numel() // N
            _bn_finalize(stats, P, gamma, beta, bn, scale, shift, mean, invstd, N, st)
        else:
            if FOLD_EVAL_BN and 0.0 <= float(cfg.slope) <= 1.0:     # eval mode: ONE launch, BatchNorm folded into weights / bias
                Wf, bf = fold_eval_bn(weight, bias, gamma, beta, bn)
                ctx.save_for_backward()
                return conv_forward_bf16(x, Wf, bf, cfg.k, cfg.stride, cfg.pad, None, cfg.name, lrelu=float(cfg.slope), out_f32=cfg.out_f32), None
            z = conv_forward_bf16(x, weight, bias, cfg.k, cfg.stride, cfg.pad, None, cfg.name)
            P = z.numel() // N
            call('cy_bn_eval_scale_shift', _ptr(gamma), _ptr(beta), _ptr(bn.running_mean), _ptr(bn.running_var), float(bn.eps),
                 _ptr(scale), _ptr(shift), N, st)
        out_f32 = cfg.out_f32
        out = torch.empty(z.shape, dtype=torch.float32 if out_f32 else torch.bfloat16, device=z.device)
        call('cy_affine_act_bf16', _ptr(z), _ptr(out), _ptr(scale), _ptr(shift), float(cfg.slope), P, N, 1 if out_f32 else 0, st)
        ctx.save_for_backward(x, weight, z, scale, shift, mean, invstd)
        if bn.training and not out_f32:
            # what the CONSUMER block's input-gradient epilogue needs for this block's BatchNorm-backward sums (bf16 output only)
            ctx.hout = BnHandover(scale, shift, mean, invstd, cfg.slope, z)
        return out, ctx.hout

    @staticmethod
    def backward(ctx, da, _hout=None):
        cfg = ctx.cfg
        if not ctx.bn_train:
            raise _lib.HipExtensionError('backward through an eval-mode BatchNorm block is not implemented')
        x, weight, z, scale, shift, mean, invstd = ctx.saved_tensors
        st = _stream()
        N = weight.shape[0]
        P = z.numel() // N
        da_f32 = da.dtype == torch.float32
        da = _f32(da, 'grad') if da_f32 else _bf(da, 'grad')
        slope = float(cfg.slope)
        given = ctx.hout.take_red() if ctx.hout is not None and not da_f32 else None
        if given is not None:
            red, slope = given[0], 1.0         # summed by the consumer block's input-gradient epilogues, which also stored da premasked
        else:
            red = _empty((N, 2), weight, torch.float64)
            call('cy_bn_bwd_reduce_bf16', _ptr(z), _ptr(da), 1 if da_f32 else 0, _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd),
                 slope, _ptr(red), P, N, st)
        red = _sync_red(red, N, st)
        dz = torch.empty_like(z)
        dgamma, dbeta = _empty((N,), weight), _empty((N,), weight)
        Bx, Hx, Wx, Cx = x.shape
        plan = conv_plan_bf16(x.shape, N, cfg.k, cfg.stride, cfg.pad, cfg.in_f32, cfg.out_f32)
        if plan.wgrad_bn and slope == 1.0 and not da_f32:
            # premasked gradient: BatchNorm-backward pass 2 inside the weight gradient's loader, dz written for the input gradient
            ws = _empty((query('cy_conv_wgrad_bf16_bn_ws_floats', Bx, z.shape[1], z.shape[2], Cx, N, cfg.k, cfg.stride),), weight)
            dW = _empty((N, Cx, cfg.k, cfg.k), weight)
            with timer.range('conv_bf16_wgrad_bn/' + cfg.name):
                call('cy_conv_wgrad_bf16_bn', _ptr(x), _ptr(da.contiguous()), _ptr(z), _ptr(dz), _ptr(dW), _ptr(ws), _ptr(scale), _ptr(mean),
                     _ptr(invstd), _ptr(red), _ptr(dgamma), _ptr(dbeta), Bx, Hx, Wx, Cx, z.shape[1], z.shape[2], N, cfg.k, cfg.stride, st)
        else:
            call('cy_bn_bwd_apply_bf16', _ptr(z), _ptr(da), 1 if da_f32 else 0, _ptr(dz), _ptr(scale), _ptr(shift), _ptr(mean),
                 _ptr(invstd), slope, _ptr(red), _ptr(dgamma), _ptr(dbeta), P, N, st)
            dW = conv_wgrad_bf16(x, dz, cfg.k, cfg.stride, cfg.pad, cfg.name)
        dbias = _const_zeros(N, weight) if ctx.has_bias else None       # in front of BatchNorm: analytically zero
        return _input_grad(ctx, dz, x, weight, plan, st), dW, dbias, dgamma, dbeta, None, None


def conv_block_bf16(x, weight, bias, gamma, beta, cfg, handover=None):
    """One bf16 conv -> BatchNorm -> LeakyReLU block: (activation, BnHandover or None).  handover: what the bf16 block in
    front returned, whose BatchNorm-backward sums this block's input-gradient kernel then leaves in it."""
    return _ConvBlockBF16.apply(x, weight, bias, gamma, beta, cfg, handover)


def conv_block(x, weight, bias, gamma, beta, cfg, handover=None):
    """One conv (+BN) (+activation) block on the fp32 kernels, as one of three Functions: without BatchNorm, the first layer's
    training block, every other BatchNorm block.  cfg.defer_act: returns (z, BnHandover) instead of the activation; the next
    block (or ops.affine_act_maxpool) then takes that object as `handover`, with z as its x, and applies the producer's
    BatchNorm + LeakyReLU on its loads (its input gradient is the gradient with respect to the ACTIVATED value, which is
    what the producer's backward expects)."""
    if cfg.bn is None:
        return _ConvBlockNoBn.apply(x, weight, bias, cfg, handover)
    plan = conv_plan(x.shape, weight.shape[0], cfg.k, cfg.stride, cfg.pad, cfg.nchw_in)
    if (plan.conv1_bwd and cfg.bn.training and not cfg.defer_act and not x.requires_grad
            and (cfg.slope is None or 0.0 <= float(cfg.slope) <= 1.0)):
        return _Conv1TrainBlock.apply(x, weight, bias, gamma, beta, cfg, plan)
    # an eval-mode block whose input wants a gradient keeps what that gradient needs (decided here: inside a Function's forward the
    # grad mode is off); under torch.no_grad() and for inputs without requires_grad nothing is kept
    eval_dx = bool(not cfg.bn.training and torch.is_grad_enabled() and x.requires_grad)
    return _ConvBnBlock.apply(x, weight, bias, gamma, beta, cfg, plan, handover, eval_dx)


# ------------------------------------------------------------------------------------------------ routing
ROUTING_FORCE_GENERAL = False   # every routing shape on the general kernels (routing_general.hip), also those the specialised kernels
#                                 take: A/B runs and cross-checks.  Read at each call, so a forward and its backward may take different paths.


ROUTING_PATHS = ('c1', 'rows_fused', 'rows_phased', 'general', 'mfma_fused', 'mfma_phased')     # CYI_ROUTE_* of csrc/common.h
ROUTING_REGIONS = ('ds_all', 'V', 'SA', 'slabs', 'tail', 'W', 'cdb', 'du_hat', 'dW_splits')      # CYI_WS_*


def routing_plan(R, N, Cc, Din, Dout, n_iter, gather_g=0, gather_B=0, backward=False, force_general=None):
    """What the library decides about one routing call (cy_routing_plan, host arithmetic): the path, the launch numbers, and the
    workspace regions [(name, offset, length)] in floats in the order they lie in, `total` being the end of the last one."""
    a = RoutingFwd(R=R, N=N, C=Cc, Din=Din, Dout=Dout, n_iter=n_iter, gather_g=gather_g, gather_B=gather_B)
    out = (C.c_longlong * (7 + 3 * len(ROUTING_REGIONS)))()
    force = ROUTING_FORCE_GENERAL if force_general is None else force_general
    rc = query('cy_routing_plan', C.byref(a), int(backward), int(force), out, len(out))
    if rc:          # no path takes the shape: the library's message says why
        msg = _lib.load().capsyolo_last_error()
        raise _lib.HipExtensionError('cy_routing_plan failed (code %d): %s' % (rc, msg.decode() if msg else '?'))
    names = [n + '_all' if backward and n == 'V' else n for n in ROUTING_REGIONS]
    return {'path': ROUTING_PATHS[out[0]], 'row_blocks': out[1], 'nch': out[2], 'ic': out[3], 'cdb': bool(out[4]), 'total': out[5],
            'regions': [(names[out[7 + 3 * k]], out[8 + 3 * k], out[9 + 3 * k]) for k in range(out[6])]}


def _routing_call(kind, a, like):
    """One plan query: the entry point of the plan's path, on a workspace of the plan's total."""
    p = routing_plan(a.R, a.N, a.C, a.Din, a.Dout, a.n_iter, a.gather_g, a.gather_B, backward=kind == 'bwd')
    ws = _empty((p['total'],), like) if p['total'] else None
    a.ws = ws.data_ptr() if p['total'] else None
    with timer.range('routing_' + kind):
        call(('cy_routing_general_' if p['path'] == 'general' else 'cy_routing_') + kind, C.byref(a), _stream())


class _Routing(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, W, n_iter, gather_g, gather_B):
        u, W = _f32(u, 'capsule input'), _f32(W, 'route_weights')
        _, N, Cc, Din, Dout = W.shape
        if gather_g:
            R = gather_g * gather_g * gather_B
            out_shape = (gather_B, gather_g, gather_g, Cc, Dout)
        else:
            R = u.shape[0]
            out_shape = (R, Cc, Dout)
        v = _empty(out_shape, u)
        s_hist = _empty((n_iter, R, Cc, Dout), u)
        _routing_call('fwd', RoutingFwd(u=u.data_ptr(), W=W.data_ptr(), v_out=v.data_ptr(), s_hist=s_hist.data_ptr(), R=R, N=N, C=Cc,
                                        Din=Din, Dout=Dout, n_iter=n_iter, gather_g=gather_g, gather_B=gather_B, ws=None), u)
        ctx.save_for_backward(u, W, s_hist)
        ctx.dims = (R, N, Cc, Din, Dout, n_iter, gather_g, gather_B)
        return v

    @staticmethod
    def backward(ctx, dv):
        u, W, s_hist = ctx.saved_tensors
        R, N, Cc, Din, Dout, n_iter, g, gB = ctx.dims
        dv = _f32(dv, 'grad')
        du, dW = torch.empty_like(u), torch.empty_like(W)
        _routing_call('bwd', RoutingBwd(u=u.data_ptr(), W=W.data_ptr(), s_hist=s_hist.data_ptr(), dv=dv.data_ptr(), du=du.data_ptr(),
                                        dW=dW.data_ptr(), ws=None, R=R, N=N, C=Cc, Din=Din, Dout=Dout, n_iter=n_iter, gather_g=g,
                                        gather_B=gB), u)
        return du, dW, None, None, None


def routing(u, W, n_iter=3, gather_g=0, gather_B=0):
    """u [R,N,Din] (or the NHWC feature map [B,4g,4g,256] with gather_g=g), W [1,N,C,Din,Dout] -> v."""
    return _Routing.apply(u, W, int(n_iter), int(gather_g), int(gather_B))


# ------------------------------------------------------------------------------------------------ small vector ops
class _Rows(torch.autograd.Function):
    """squash / length over the last dimension."""

    @staticmethod
    def forward(ctx, x, kind):
        x = _f32(x)
        D = x.shape[-1]
        rows = x.numel() // D
        st = _stream()
        ctx.kind = kind
        if kind == 'squash':
            y = torch.empty_like(x)
            call('cy_squash_fwd', _ptr(x), _ptr(y), rows, D, st)
            ctx.save_for_backward(x)
        else:
            y = _empty(x.shape[:-1], x)
            call('cy_length_fwd', _ptr(x), _ptr(y), rows, D, st)
            ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _f32(dy)
        st = _stream()
        x = ctx.saved_tensors[0]
        D = x.shape[-1]
        rows = x.numel() // D
        dx = torch.empty_like(x)
        if ctx.kind == 'squash':
            call('cy_squash_bwd', _ptr(x), _ptr(dy), _ptr(dx), rows, D, st)
        else:
            call('cy_length_bwd', _ptr(x), _ptr(ctx.saved_tensors[1]), _ptr(dy), _ptr(dx), rows, D, st)
        return dx, None


def squash(x):
    return _Rows.apply(x, 'squash')


def length(x):
    return _Rows.apply(x, 'length')


class _Permute4(torch.autograd.Function):
    """out[b][i1][i2][i3] = in[b*sb + i1*s1 + i2*s2 + i3*s3]; backward is the inverse scatter."""

    @staticmethod
    def forward(ctx, x, nb, dims, strides):
        x = _f32(x)
        out = _empty((nb,) + tuple(dims), x)
        call('cy_permute4', _ptr(x), _ptr(out), nb, dims[0], dims[1], dims[2], strides[0], strides[1], strides[2],
             strides[3], 0, _stream())
        ctx.args = (nb, dims, strides, tuple(x.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        nb, dims, strides, xshape = ctx.args
        dout = _f32(dout)
        dx = _empty(xshape, dout)
        call('cy_permute4', _ptr(dout), _ptr(dx), nb, dims[0], dims[1], dims[2], strides[0], strides[1], strides[2],
             strides[3], 1, _stream())
        return dx, None, None, None


def nchw_to_nhwc(x):
    B, Cc, H, W = x.shape
    return _Permute4.apply(x, B, (H, W, Cc), (Cc * H * W, W, 1, H * W))


def nhwc_to_nchw(x):
    B, H, W, Cc = x.shape
    return _Permute4.apply(x, B, (Cc, H, W), (H * W * Cc, 1, W * Cc, Cc))


def primary_caps_rows(z, n_caps):
    """conv output [B,h,w,(o,cap)] -> capsule rows [B, o*h*w + y*w + x, cap] (models.py:81: view(B,-1,1) + cat)."""
    B, H, W, Cc = z.shape
    O = Cc // n_caps
    out = _Permute4.apply(z, B, (O, H * W, n_caps), (H * W * Cc, n_caps, Cc, 1))
    return out.view(B, O * H * W, n_caps)


class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        B, H, W, Cc = x.shape
        Ho, Wo = H // 2, W // 2                  # nn.MaxPool2d(2) floors: the last row / column of an odd map is ignored
        y = _empty((B, Ho, Wo, Cc), x)
        idx = _empty((B, Ho, Wo, Cc), x, torch.uint8)
        ctx.shape = (B, H, W, Cc)
        ctx.save_for_backward(idx)
        if y.numel() == 0:                       # a map of one row or column: nothing to launch
            return y
        if H != 2 * Ho or W != 2 * Wo:           # the kernels address [B][2 Ho][2 Wo][C]: hand them exactly that
            x = x[:, :2 * Ho, :2 * Wo].contiguous()
        call('cy_maxpool2_fwd', _ptr(x), _ptr(y), _ptr(idx), B, Ho, Wo, Cc, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        B, H, W, Cc = ctx.shape
        Ho, Wo = H // 2, W // 2
        dy = _f32(dy)
        if idx.numel() == 0:
            return torch.zeros((B, H, W, Cc), device=dy.device)
        dx = _empty((B, 2 * Ho, 2 * Wo, Cc), dy)
        call('cy_maxpool2_bwd', _ptr(dy), _ptr(idx), _ptr(dx), B, Ho, Wo, Cc, _stream())
        if H != 2 * Ho or W != 2 * Wo:           # the ignored row / column gets a gradient of zero
            full = torch.zeros((B, H, W, Cc), device=dy.device)
            full[:, :2 * Ho, :2 * Wo] = dx
            dx = full
        return dx


def maxpool2(x):
    return _MaxPool2.apply(x)


FUSE_POOL = True    # conv -> BatchNorm -> LeakyReLU -> MaxPool blocks (DarkNet): activation + pooling in one pass over z, pooling backward +
                    # the block's BatchNorm-backward sums in one pass (the full-resolution activation and its gradient are never stored twice)


def pool_fusable(C, H, W, slope):
    """The fused BatchNorm-apply + LeakyReLU + 2x2 max-pool pass takes this block's output [B,H,W,C]."""
    return (FUSE_POOL and H % 2 == 0 and W % 2 == 0 and C % 4 == 0 and (C % 64 == 0 or C in (4, 8, 16, 32)) and slope is not None
            and 0.0 < slope <= 1.0)


class _AffineActMaxPool(torch.autograd.Function):
    """y = maxpool2(lrelu(z * scale + shift)) of a block that deferred its activation (ConvBlockCfg.defer_act); plays the CONSUMER of the
    producer's BnHandover h: its backward returns the premasked gradient d = [pos == argmax] dy lrelu'(.) as the gradient of z and gives
    the producer's BatchNorm-backward sums to h (models.py:135 ... 195: nn.LeakyReLU + nn.MaxPool2d of the DarkNet blocks)."""

    @staticmethod
    def forward(ctx, z, h):
        z = _f32(z, 'conv output')
        B, H, W, Cc = z.shape
        y = _empty((B, H // 2, W // 2, Cc), z)
        idx = torch.empty((B, H // 2, W // 2, Cc), dtype=torch.uint8, device=z.device)
        with timer.range('affine_act_maxpool'):
            call('cy_affine_act_maxpool2', _ptr(z), _ptr(h.scale), _ptr(h.shift), h.slope, _ptr(y), _ptr(idx), B, H // 2, W // 2, Cc, _stream())
        ctx.save_for_backward(z, idx)
        ctx.h = h
        return y

    @staticmethod
    def backward(ctx, dy):
        z, idx = ctx.saved_tensors
        B, H, W, Cc = z.shape
        dy = _f32(dy, 'pooled gradient')
        h = ctx.h
        d = torch.empty_like(z)
        red = zero_pool.take((Cc, 2), torch.float64, z.device)
        with timer.range('maxpool_bwd_bn'):
            call('cy_maxpool2_bwd_bn', _ptr(dy), _ptr(idx), _ptr(z), _ptr(h.scale), _ptr(h.shift), _ptr(h.mean), _ptr(h.invstd), h.slope,
                 _ptr(d), _ptr(red), B, H // 2, W // 2, Cc, _stream())
        h.give_red(red, True)
        return d, None


def affine_act_maxpool(z, handover):
    return _AffineActMaxPool.apply(z, handover)


class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f):
        x = _f32(x)
        B, H, W, Cc = x.shape
        y = _empty((B, H * f, W * f, Cc), x)
        call('cy_upsample_fwd', _ptr(x), _ptr(y), B, H, W, Cc, f, _stream())
        ctx.args = (B, H, W, Cc, f)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Cc, f = ctx.args
        dy = _f32(dy)
        dx = _empty((B, H, W, Cc), dy)
        call('cy_upsample_bwd', _ptr(dy), _ptr(dx), B, H, W, Cc, f, _stream())
        return dx, None


def upsample_nearest(x, f):
    return _Upsample.apply(x, int(f))


class _Tanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        y = torch.empty_like(x)
        call('cy_tanh_fwd', _ptr(x), _ptr(y), x.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _f32(dy)
        dx = torch.empty_like(y)
        call('cy_tanh_bwd', _ptr(y), _ptr(dy), _ptr(dx), y.numel(), _stream())
        return dx


def tanh(x):
    return _Tanh.apply(x)


class _YoloHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, split, n_classes):
        x = _f32(x)
        y = torch.empty_like(x)
        cells = x.numel() // (split + n_classes)
        call('cy_yolo_head_fwd', _ptr(x), _ptr(y), cells, split, n_classes, _stream())
        ctx.save_for_backward(y)
        ctx.args = (cells, split, n_classes)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        cells, split, n_classes = ctx.args
        dy = _f32(dy)
        dx = torch.empty_like(y)
        call('cy_yolo_head_bwd', _ptr(y), _ptr(dy), _ptr(dx), cells, split, n_classes, _stream())
        return dx, None, None


def yolo_head(x, split, n_classes):
    return _YoloHead.apply(x, int(split), int(n_classes))


class _PickCapsule(torch.autograd.Function):
    @staticmethod
    def forward(ctx, caps, y):
        caps = _f32(caps)
        B, Cc, D = caps.shape
        y = y.to(torch.int64).contiguous()
        out = _empty((B, D), caps)
        call('cy_pick_capsule', _ptr(caps), _ptr(y), _ptr(out), B, Cc, D, 0, _stream())
        ctx.save_for_backward(y)
        ctx.shape = (B, Cc, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        (y,) = ctx.saved_tensors
        B, Cc, D = ctx.shape
        dout = _f32(dout)
        dcaps = _empty((B, Cc, D), dout)
        call('cy_pick_capsule', _ptr(dout), _ptr(y), _ptr(dcaps), B, Cc, D, 1, _stream())
        return dcaps, None


def pick_capsule(caps, y):
    return _PickCapsule.apply(caps, y)


# ------------------------------------------------------------------------------------------------ losses
def _scaled(grad, gout):
    out = torch.empty_like(grad)
    gout = gout.to(torch.float32).contiguous()
    call('cy_scale_by_device_scalar', _ptr(grad), _ptr(gout), _ptr(out), grad.numel(), _stream())
    return out


class _DarkCapsuleLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, caps, y):
        caps = _f32(caps, 'caps')
        if caps.shape[-1] != 5 or y.shape[-1] < 5 or tuple(y.shape[:-1]) != tuple(caps.shape[:-1]):
            raise _lib.HipExtensionError('darkcapsule_loss: caps must be [B,g,g,5] and the labels [B,g,g,>=5] on the same grid; got %s and %s'
                                         % (tuple(caps.shape), tuple(y.shape)))
        if not (y.is_cuda and y.dtype == torch.float64):
            y = y.to(device=caps.device, dtype=torch.float64)
        y = y.contiguous()
        B = caps.shape[0]
        cells = caps.numel() // (5 * B)
        loss, dcaps = _empty((), caps), torch.empty_like(caps)
        call('cy_darkcapsule_loss', _ptr(caps), _ptr(y), y.shape[-1], _ptr(loss), _ptr(dcaps), B, cells, _stream())
        ctx.save_for_backward(dcaps)
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _scaled(ctx.saved_tensors[0], gout), None


class _DarkCapsule23Loss(torch.autograd.Function):
    """darkcapsule2_loss (caps [B,g,g,5+C]) / darkcapsule3_loss (caps [B,g,g,C,D]); loss_fns.py:145-184."""

    @staticmethod
    def forward(ctx, caps, y, variant):
        caps = _f32(caps, 'caps')
        if y.dim() != 4 or y.shape[-1] < 5 or tuple(caps.shape[:3]) != tuple(y.shape[:3]):
            raise _lib.HipExtensionError('darkcapsule%d_loss: the labels must be [B,g,g,5+n_classes] on the grid of the capsules; got %s '
                                         'and capsules %s' % (variant, tuple(y.shape), tuple(caps.shape)))
        if not (y.is_cuda and y.dtype == torch.float64):
            y = y.to(device=caps.device, dtype=torch.float64)
        y = y.contiguous()
        B = caps.shape[0]
        Cc = y.shape[-1] - 5
        cells = y.numel() // (y.shape[-1] * B)
        loss, dcaps = _empty((), caps), torch.empty_like(caps)
        if variant == 2:
            if caps.dim() != 4 or caps.shape[-1] != 5 + Cc:
                raise _lib.HipExtensionError('darkcapsule2_loss: caps last dim %d != 5 + n_classes %d' % (caps.shape[-1], Cc))
            call('cy_darkcapsule2_loss', _ptr(caps), _ptr(y), _ptr(loss), _ptr(dcaps), B, cells, Cc, _stream())
        else:
            if caps.dim() != 5 or caps.shape[3] != Cc:
                raise _lib.HipExtensionError('darkcapsule3_loss: caps must be [B,g,g,n_classes,D]; got %s' % (tuple(caps.shape),))
            call('cy_darkcapsule3_loss', _ptr(caps), _ptr(y), _ptr(loss), _ptr(dcaps), B, cells, Cc, caps.shape[4], _stream())
        ctx.save_for_backward(dcaps)
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _scaled(ctx.saved_tensors[0], gout), None, None


def darkcapsule2_loss_fn(caps, y):
    return _DarkCapsule23Loss.apply(caps, y, 2)


def darkcapsule3_loss_fn(caps, y):
    return _DarkCapsule23Loss.apply(caps, y, 3)


class _CapsuleLoss(torch.autograd.Function):
    """margin loss (+ recon_coef * sum (x - recon)^2), all divided by B."""

    @staticmethod
    def forward(ctx, scores, y, x, recon, coef):
        scores = _f32(scores, 'scores')
        B, Cc = scores.shape
        y = y.to(torch.int64).contiguous()
        st = _stream()
        loss, dscores = _empty((), scores), torch.empty_like(scores)
        call('cy_margin_loss', _ptr(scores), _ptr(y), _ptr(loss), _ptr(dscores), B, Cc, st)
        if recon is not None:
            x, recon = _f32(x, 'x'), _f32(recon, 'recon')
            drecon = torch.empty_like(recon)
            call('cy_recon_loss_add', _ptr(x), _ptr(recon), float(coef) / B, _ptr(loss), _ptr(drecon), recon.numel(), st)
            ctx.save_for_backward(dscores, drecon)
        else:
            ctx.save_for_backward(dscores)
        return loss

    @staticmethod
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        drecon = _scaled(saved[1], gout) if len(saved) > 1 else None
        return _scaled(saved[0], gout), None, None, drecon, None


class _DarkLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pred, y_true, nb, n_classes, l_coord, l_noobj, img):
        y_pred = _f32(y_pred, 'y_pred')
        nb, n_classes = int(nb), int(n_classes)
        B, g = y_pred.shape[0], (y_pred.shape[1] if y_pred.dim() > 1 else 0)
        # the kernel strides y_pred by 5 n_boxes + n_classes and y_true by 5 + n_classes over B g g cells
        if tuple(y_pred.shape) != (B, g, g, 5 * nb + n_classes) or y_true.dim() != 4 or tuple(y_true.shape[:3]) != (B, g, g):
            raise _lib.HipExtensionError('dark_loss: y_pred must be [B,g,g,5*%d+%d] and y_true [B,g,g,5+%d] on the same grid; got %s and %s'
                                         % (nb, n_classes, n_classes, tuple(y_pred.shape), tuple(y_true.shape)))
        if y_true.shape[-1] != 5 + n_classes:
            if n_classes != 0 or y_true.shape[-1] < 5:
                raise _lib.HipExtensionError('dark_loss: labels of %d columns with n_classes = %d' % (y_true.shape[-1], n_classes))
            y_true = y_true[..., :5]                             # recognition-model labels: without classes only these columns are read
        if not (y_true.is_cuda and y_true.dtype == torch.float64):
            y_true = y_true.to(device=y_pred.device, dtype=torch.float64)
        y_true = y_true.contiguous()
        loss, avg_iou = _empty((), y_pred), _empty((), y_pred)
        dpred = torch.empty_like(y_pred)
        call('cy_dark_loss', _ptr(y_pred), _ptr(y_true), _ptr(loss), _ptr(avg_iou), _ptr(dpred), B, g, nb, n_classes,
             float(l_coord), float(l_noobj), float(img), _stream())
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(avg_iou)
        return loss, avg_iou

    @staticmethod
    def backward(ctx, gout, _g_iou):
        return _scaled(ctx.saved_tensors[0], gout), None, None, None, None, None, None


def darkcapsule_loss_fn(caps, y):
    return _DarkCapsuleLoss.apply(caps, y)


def capsule_loss_fn(scores, y, x=None, recon=None, coef=0.0):
    return _CapsuleLoss.apply(scores, y, x, recon, coef)


def dark_loss_fn(y_pred, y_true, nb, n_classes, l_coord, l_noobj, img):
    return _DarkLoss.apply(y_pred, y_true, nb, n_classes, l_coord, l_noobj, img)


# ------------------------------------------------------------------------------------------------ linear layers, cross-entropy
LINEAR_MAX_M, LINEAR_MAX_N, LINEAR_MAX_K, XENT_MAX_C = 4096, 1024, 1 << 20, 1024     # the range of csrc/linear.hip


def _linear_shape_ok(who, M, N, K):
    if not (1 <= M <= LINEAR_MAX_M and 1 <= N <= LINEAR_MAX_N and 4 <= K <= LINEAR_MAX_K and K % 4 == 0):
        raise _lib.HipExtensionError('%s: M=%d N=%d K=%d is outside the linear kernels\' range (M 1..%d, N 1..%d, K a multiple of 4 up '
                                     'to %d); there is no other path' % (who, M, N, K, LINEAR_MAX_M, LINEAR_MAX_N, LINEAR_MAX_K))


def _f32_16(t, name):
    """_f32 and 16-byte aligned (the kernels load and store rows of K floats 16 bytes at a time)."""
    t = _f32(t, name)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def linear_shares(M, N, K):
    """(shares, slice, workspace floats) of cy_linear_fwd for the shape: host arithmetic, answered without a device."""
    return query('cy_linear_fwd_shares', M, N, K), query('cy_linear_fwd_slice', M, N, K), query('cy_linear_fwd_ws_floats', M, N, K)


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b) on csrc/linear.hip.  x_relu: x is the output of a ReLU; dx is then zeroed where x <= 0 in the store of the
    input-gradient kernel, which is that ReLU's backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, x_relu):
        M, K = x.shape
        N = weight.shape[0]
        st = _stream()
        y = _empty((M, N), x)
        nws = query('cy_linear_fwd_ws_floats', M, N, K)
        ws = _empty((nws,), x) if nws else None               # torch's allocator: nothing is allocated by the kernels (graph capture)
        with timer.range('linear_fwd'):
            call('cy_linear_fwd', _ptr(x), _ptr(weight), _ptr(bias), _ptr(y), M, N, K, 1 if relu else 0, _ptr(ws), st)
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.relu, ctx.x_relu, ctx.has_bias = relu, x_relu, bias is not None
        ctx.masked_by_consumer = False                        # set by linear(): the next layer's dgrad applies this layer's ReLU backward
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        M, K = x.shape
        N = weight.shape[0]
        st = _stream()
        dy = _f32(dy, 'dy')
        if ctx.relu and not ctx.masked_by_consumer:
            dz = torch.empty_like(dy)
            call('cy_act_bwd', _ptr(y), _ptr(dy), _ptr(dz), 0.0, dy.numel(), st)
            dy = dz
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            with timer.range('linear_dgrad'):
                call('cy_linear_dgrad', _ptr(dy), _ptr(weight), _ptr(dx), _ptr(x) if ctx.x_relu else None, M, N, K, st)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty_like(weight)
            db = _empty((N,), x) if ctx.has_bias else None
            with timer.range('linear_wgrad'):
                call('cy_linear_wgrad', _ptr(dy), _ptr(x), _ptr(dw), _ptr(db), M, N, K, st)
        return dx, dw, db, None, None


def linear(x, weight, bias, relu=False):
    """F.linear(x, weight, bias), followed by ReLU with ``relu``, as ONE autograd.Function on the kernels of csrc/linear.hip
    (x [M,K], weight [N,K], bias [N] or None; fp32 on the GPU).  A layer with ``relu`` saves its output.  When that output is the
    ``x`` of the next ``linear`` call, the ReLU's backward is the mask in the store of the next layer's input-gradient kernel
    (``dx = 0 where x <= 0``), and this layer takes the gradient as it arrives; for any other consumer this layer masks the gradient
    itself (cy_act_bwd) -- so a ``relu`` output must not feed a ``linear`` call AND another consumer at once."""
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1] or (bias is not None and tuple(bias.shape) != (weight.shape[0],)):
        raise _lib.HipExtensionError('linear: x [M,K], weight [N,K], bias [N] expected; got %s, %s, %s'
                                     % (tuple(x.shape), tuple(weight.shape), None if bias is None else tuple(bias.shape)))
    _linear_shape_ok('linear', x.shape[0], weight.shape[0], x.shape[1])
    producer = x.grad_fn if isinstance(x.grad_fn, _Linear._backward_cls) and x.grad_fn.relu else None
    xa = _f32_16(x, 'x')
    x_relu = producer is not None and xa is x and torch.is_grad_enabled()
    y = _Linear.apply(xa, _f32_16(weight, 'weight'), None if bias is None else _f32(bias, 'bias'), bool(relu), x_relu)
    if x_relu and y.requires_grad:
        producer.masked_by_consumer = True
    return y


class _SoftmaxXent(torch.autograd.Function):
    """loss_fns.py:6-8: mean over the batch of -log softmax(scores)[y]; value and gradient in one launch."""

    @staticmethod
    def forward(ctx, scores, y):
        M, Cc = scores.shape
        loss, dscores = _empty((), scores), torch.empty_like(scores)
        call('cy_softmax_xent', _ptr(scores), _ptr(y), _ptr(loss), _ptr(dscores), M, Cc, _stream())
        ctx.save_for_backward(dscores)
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _scaled(ctx.saved_tensors[0], gout), None


def softmax_xent_fn(scores, y):
    if scores.dim() != 2 or y.dim() != 1 or y.shape[0] != scores.shape[0]:
        raise _lib.HipExtensionError('softmax_xent: scores [M,C] and y [M] expected; got %s, %s' % (tuple(scores.shape), tuple(y.shape)))
    M, Cc = scores.shape
    if not (1 <= M <= LINEAR_MAX_M and 1 <= Cc <= XENT_MAX_C):
        raise _lib.HipExtensionError('softmax_xent: M=%d C=%d is outside the kernel\'s range (M 1..%d, C 1..%d)'
                                     % (M, Cc, LINEAR_MAX_M, XENT_MAX_C))
    scores = _f32(scores, 'scores')
    return _SoftmaxXent.apply(scores, y.to(device=scores.device, dtype=torch.int64).contiguous())

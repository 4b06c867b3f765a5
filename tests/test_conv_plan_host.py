"""The fp32 convolution's plan (ops.conv_plan): which kernel family runs the forward, the input gradient and the weight gradient of a
layer, and what its block may fuse.  Host arithmetic: no GPU.  The rows of the measured configurations (BASELINE configs[2], the
loss-curve recipes, darknet_d, CapsuleNet) are pinned literally, taken from the predicates this function replaced; a change of any of
them is a change of which kernel runs a measured configuration and has to be made here on purpose."""
import itertools

import pytest

from helpers import REPO  # noqa: F401  (puts the repository on sys.path)

from capsyolo_amd import ops

FLAGS = ('in_affine', 'dgrad_bn_fuse', 'dgrad_premasks', 'wgrad_bn', 'wgrad_bn4', 'conv1', 'conv1_bwd', 'conv1_moments', 'conv1_onepass')
SWITCHES = ('USE_WINOGRAD', 'USE_WINOGRAD4', 'USE_WINOGRAD4_WGRAD', 'USE_WINOGRAD_S2', 'USE_WINOGRAD_S2_DGRAD', 'USE_WINOGRAD4_S2',
            'USE_WINOGRAD4_S2_DGRAD', 'USE_CONV1', 'USE_CONV1_BWD', 'USE_CONV1_MOMENTS', 'USE_CONV1_ONEPASS', 'FUSE_BN_BWD_REDUCE',
            'FUSE_BN_BWD_APPLY')


def row(*args, **kw):
    """(forward, input gradient, weight gradient, names of the facts that hold): a plan as one readable tuple."""
    p = ops.conv_plan(*args, **kw)
    return (p.fwd, p.dgrad, p.wgrad, ' '.join(f for f in FLAGS if getattr(p, f)))


def test_switch_defaults():
    """The rows below are the plans of the DEFAULT switches and thresholds."""
    assert all(getattr(ops, s) is True for s in SWITCHES) and ops.FUSE_INPUT_AFFINE is True
    assert (ops.WINOGRAD4_MIN_PIXELS, ops.WINOGRAD4_S2_MIN_PIXELS, ops.CONV1_MOMENTS_MIN_PIXELS) == (1 << 17, 1 << 16, 1 << 18)


# ------------------------------------------------------------------------------------------------ the measured configurations
CONV1 = ('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_moments conv1_onepass')
F43 = ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wino4_wgrad', 'wgrad_bn wgrad_bn4')
F42 = ('conv_wino42_fwd', 'conv_wino42_dgrad', 'conv_wino2_wgrad', 'in_affine dgrad_bn_fuse dgrad_premasks')
F22S2 = ('conv_wino2_fwd', 'conv_wino2_dgrad', 'conv_wino2_wgrad', 'in_affine dgrad_bn_fuse dgrad_premasks')
# recipe -> (image side, batch, rows of conv_1 .. conv_5 of models._darkcaps_backbone)
DARKCAPS = {
    'headline 416 x 416, batch 32 (BASELINE configs[2])': (416, 32, [CONV1, F43, F42, F42, F42]),
    'dw64': (64, 64, [CONV1, F43, F42, F22S2, F22S2]),
    'di96': (96, 8, [('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_onepass'),
                     ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wino_wgrad', 'wgrad_bn'), F22S2, F22S2, F22S2]),
    'di256': (256, 4, [CONV1, F43, F42, F22S2, F22S2]),
}


def darkcaps_rows(H, B, **kw):
    return [row((B, 3, H, H), 128, 3, 1, 1, True, **kw), row((B, H, H, 128), 256, 3, 1, 1, **kw), row((B, H, H, 256), 64, 4, 2, 1, **kw),
            row((B, H // 2, H // 2, 64), 128, 4, 2, 1, **kw), row((B, H // 4, H // 4, 128), 256, 4, 2, 1, **kw)]


@pytest.mark.parametrize('recipe', sorted(DARKCAPS))
def test_darkcapsule_backbone_keeps_its_plan(recipe):
    H, B, want = DARKCAPS[recipe]
    assert darkcaps_rows(H, B) == want


F43_F22W = ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wino_wgrad', 'wgrad_bn')
F22 = ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wino_wgrad', 'wgrad_bn')
GEMM = ('conv_gemm_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')
# darknet_d at 416 x 416, batch 16 (models._DARKNET_PLAN + conv_19): (map side, Cin, Cout, k) -> row
DARKNET = [
    ((416, 3, 32, 3), CONV1),
    ((208, 32, 64, 3), ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wino4_wgrad', '')),     # Cin = 32: no fused BatchNorm-apply form
    ((104, 64, 128, 3), F43_F22W), ((104, 128, 64, 1), GEMM), ((104, 64, 128, 3), F43_F22W),
    ((52, 128, 256, 3), F22), ((52, 256, 128, 1), GEMM), ((52, 128, 256, 3), F22),
    ((26, 256, 512, 3), F22), ((26, 512, 256, 1), GEMM), ((26, 256, 512, 3), F22), ((26, 512, 256, 1), GEMM), ((26, 256, 512, 3), F22),
    ((13, 512, 1024, 3), F22), ((13, 1024, 512, 1), GEMM), ((13, 512, 1024, 3), F22), ((13, 1024, 512, 1), GEMM),
    ((13, 512, 1024, 3), F22), ((13, 1024, 10, 1), GEMM),
]


def test_darknet_d_keeps_its_plan():
    for i, ((H, cin, cout, k), want) in enumerate(DARKNET):
        shape = (16, cin, H, H) if i == 0 else (16, H, H, cin)
        assert row(shape, cout, k, 1, k // 2, i == 0) == want, (i + 1, H, cin, cout, k)


def test_capsulenet_keeps_its_plan():
    """experiments/capsule, 32 x 32, batch 32, reconstruction on: nothing but the implicit GEMM / direct kernels, except three
    small 3x3 layers of the decoder whose channel counts (multiples of 8) let one pass onto F(2x2,3x3)."""
    B = 32
    assert row((B, 3, 32, 32), 256, 9, 1, 0, True, relu=True) == ('conv_gemm_fwd', None, 'conv_wgrad', '')                     # conv1
    assert row((B, 24, 24, 256), 128, 8, 2, 0) == GEMM                                                                         # primary_caps
    assert row((B, 1, 1, 16), 256, 1, 1, 0, relu=True) == GEMM                                                                 # dec_fc
    assert row((B, 8, 8, 16), 4, 3, 1, 1, relu=True) == GEMM                                                                   # dec_4
    assert row((B, 16, 16, 4), 8, 3, 1, 1, relu=True) == ('conv_gemm_fwd', 'conv_wino_dgrad', 'conv_wgrad', '')                # dec_7
    assert row((B, 32, 32, 8), 16, 3, 1, 1, relu=True) == ('conv_gemm_fwd', 'conv_wino_dgrad', 'conv_wgrad', '')               # dec_10
    assert row((B, 32, 32, 16), 3, 3, 1, 1) == ('conv_wino_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')             # dec_12


# ------------------------------------------------------------------------------------------------ boundaries
def test_pixel_thresholds():
    # WINOGRAD4_MIN_PIXELS = 2^17 output pixels: forward, input gradient, weight gradient and the fused form's F(3x3,4x4) variant move together
    assert row((2, 256, 256, 64), 64, 3, 1, 1) == F43
    assert row((1, 512, 256, 64), 64, 3, 1, 1) == F43
    assert row((1, 512, 252, 64), 64, 3, 1, 1) == F22                       # 129024 pixels (and W not a multiple of 16)
    assert row((1, 508, 256, 64), 64, 3, 1, 1) == F22                       # 130048 pixels, every shape condition of F(3x3,4x4) met
    # WINOGRAD4_S2_MIN_PIXELS = 2^16 OUTPUT pixels
    assert row((1, 512, 512, 64), 64, 4, 2, 1) == F42
    assert row((1, 512, 510, 64), 64, 4, 2, 1) == F22S2                     # 65280
    # CONV1_MOMENTS_MIN_PIXELS = 2^18 input pixels
    assert row((1, 3, 512, 512), 64, 3, 1, 1, True) == CONV1
    assert row((1, 3, 511, 512), 64, 3, 1, 1, True) == ('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_onepass')


@pytest.mark.parametrize('name,shape,cout,k,nchw,field', [
    ('WINOGRAD4_MIN_PIXELS', (3, 20, 32, 64), 64, 3, False, 'fwd'), ('WINOGRAD4_MIN_PIXELS', (3, 20, 32, 64), 64, 3, False, 'dgrad'),
    ('WINOGRAD4_MIN_PIXELS', (3, 20, 32, 64), 64, 3, False, 'wgrad'), ('WINOGRAD4_MIN_PIXELS', (3, 20, 32, 64), 64, 3, False, 'wgrad_bn4'),
    ('WINOGRAD4_S2_MIN_PIXELS', (3, 40, 64, 64), 64, 4, False, 'fwd'), ('WINOGRAD4_S2_MIN_PIXELS', (3, 40, 64, 64), 64, 4, False, 'dgrad'),
    ('CONV1_MOMENTS_MIN_PIXELS', (3, 3, 20, 32), 64, 3, True, 'conv1_moments')])
def test_each_threshold_at_n_minus_one_and_n(name, shape, cout, k, nchw, field, monkeypatch):
    """1920 pixels each (3 x 20 x 32; the stride-2 layer's OUTPUT): the threshold at 1920 takes the layer, at 1921 leaves it."""
    s, p = (2, 1) if k == 4 else (1, 1)
    monkeypatch.setattr(ops, name, 1920)
    on = getattr(ops.conv_plan(shape, cout, k, s, p, nchw), field)
    monkeypatch.setattr(ops, name, 1921)
    off = getattr(ops.conv_plan(shape, cout, k, s, p, nchw), field)
    assert (on, off) == {'fwd': ('conv_wino4%s_fwd' % ('2' if k == 4 else ''), 'conv_wino%s_fwd' % ('2' if k == 4 else '')),
                         'dgrad': ('conv_wino4%s_dgrad' % ('2' if k == 4 else ''), 'conv_wino%s_dgrad' % ('2' if k == 4 else '')),
                         'wgrad': ('conv_wino4_wgrad', 'conv_wino_wgrad'), 'wgrad_bn4': (True, False), 'conv1_moments': (True, False)}[field]


def fams(shape, cout, k, s, p, nchw=False, **kw):
    return row(shape, cout, k, s, p, nchw, **kw)[:3]


def test_channel_boundaries_3x3():
    B, H = 2, 32                                            # 2048 pixels: the F(2x2,3x3) / F(3x3,2x2) side of the pixel threshold
    assert fams((B, H, H, 8), 8, 3, 1, 1) == ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wgrad')
    assert fams((B, H, H, 4), 8, 3, 1, 1) == ('conv_gemm_fwd', 'conv_wino_dgrad', 'conv_wgrad')           # forward: Cin % 8
    assert fams((B, H, H, 12), 8, 3, 1, 1) == ('conv_gemm_fwd', 'conv_wino_dgrad', 'conv_wgrad')
    assert fams((B, H, H, 8), 4, 3, 1, 1) == ('conv_wino_fwd', 'conv_gemm_dgrad', 'conv_wgrad')           # input gradient: Cout % 8
    assert fams((B, H, H, 8), 12, 3, 1, 1) == ('conv_wino_fwd', 'conv_gemm_dgrad', 'conv_wgrad')
    assert row((B, H, H, 64), 64, 3, 1, 1) == F22                                                         # weight gradient: both % 64
    assert row((B, H, H, 32), 64, 3, 1, 1) == ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wgrad', '')
    assert row((B, H, H, 64), 96, 3, 1, 1) == ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wgrad', '')
    # F(3x3,4x4) (cy_wino4_wgrad_ok): Cin % 32, Cout % 64, H % 4, W % 16 -- wider than F(3x3,2x2) in Cin, but without the fused form there
    B, H = 2, 256
    assert row((B, H, H, 32), 64, 3, 1, 1) == ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wino4_wgrad', '')
    assert row((B, H, H, 16), 64, 3, 1, 1) == ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wgrad', '')
    assert row((B, H, H, 32), 32, 3, 1, 1) == ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wgrad', '')
    assert row((B, 258, 256, 64), 64, 3, 1, 1) == F43_F22W                                               # H % 4
    assert row((B, 256, 264, 64), 64, 3, 1, 1) == F43_F22W                                               # W % 16
    # the geometry: 3x3 / stride 1 / pad 1 only, NHWC only
    for k, s, p in ((3, 1, 0), (3, 2, 1), (5, 1, 1), (1, 1, 1)):
        assert row((B, H, H, 64), 64, k, s, p) == GEMM, (k, s, p)
    assert row((B, 64, H, H), 64, 3, 1, 1, True) == ('conv_gemm_fwd', None, 'conv_wgrad', '')
    # the fused ReLU epilogue is the implicit GEMM's alone; the LeakyReLU epilogue (eval forward) is also Winograd's
    assert fams((B, H, H, 64), 64, 3, 1, 1, relu=True) == ('conv_gemm_fwd', 'conv_wino4_dgrad', 'conv_wino4_wgrad')
    assert fams((B, H, H, 64), 64, 3, 1, 1, lrelu=True) == F43[:3]


def test_channel_boundaries_4x4_stride_2():
    B, H = 2, 32
    assert row((B, H, H, 64), 64, 4, 2, 1) == F22S2
    assert row((B, H, H, 8), 8, 4, 2, 1) == ('conv_wino2_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')          # forward: Cin % 8
    assert row((B, H, H, 4), 8, 4, 2, 1) == GEMM
    assert row((B, H, H, 64), 8, 4, 2, 1) == ('conv_wino2_fwd', 'conv_wino2_dgrad', 'conv_wgrad', 'dgrad_bn_fuse dgrad_premasks')
    assert row((B, H, H, 32), 8, 4, 2, 1) == ('conv_wino2_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')        # input gradient: Cin % 64
    assert row((B, H, H, 64), 4, 4, 2, 1) == ('conv_wino2_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')        # ... and Cout % 8
    assert row((B, H, H, 32), 64, 4, 2, 1) == ('conv_wino2_fwd', 'conv_gemm_dgrad', 'conv_wino2_wgrad', 'in_affine dgrad_bn_fuse')   # weight gradient:
    assert row((B, H, H, 16), 64, 4, 2, 1) == ('conv_wino2_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')       # Cin % 32, Cout % 64
    assert row((B, H, H, 64), 32, 4, 2, 1) == ('conv_wino2_fwd', 'conv_wino2_dgrad', 'conv_wgrad', 'dgrad_bn_fuse dgrad_premasks')
    for shape in ((B, 31, 32, 64), (B, 32, 31, 64)):                                                                    # even maps only
        assert row(shape, 64, 4, 2, 1) == GEMM
    for k, s, p in ((4, 2, 0), (4, 1, 1), (2, 2, 1)):
        assert row((B, H, H, 64), 64, k, s, p) == GEMM, (k, s, p)
    assert row((B, H, H, 64), 64, 4, 2, 1, relu=True) == ('conv_gemm_fwd', 'conv_wino2_dgrad', 'conv_wino2_wgrad', 'dgrad_bn_fuse dgrad_premasks')
    # the producer's BatchNorm-backward sums need Cin % 4 (and never ride a 3x3 Winograd input gradient)
    assert row((B, H, H, 6), 64, 4, 2, 1) == ('conv_gemm_fwd', 'conv_gemm_dgrad', 'conv_wgrad', '')
    assert row((B, H, H, 6), 64, 1, 1, 0) == ('conv_gemm_fwd', 'conv_gemm_dgrad', 'conv_wgrad', '')


def test_first_layer_shapes():
    soft = ('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_onepass')                 # (2048 pixels: below the moment threshold)
    for cout in (32, 64, 128):
        assert row((2, 3, 32, 32), cout, 3, 1, 1, True) == soft
    nothing = ('conv_gemm_fwd', None, 'conv_wgrad', '')
    for cout in (16, 96, 256):
        assert row((2, 3, 32, 32), cout, 3, 1, 1, True) == nothing
    assert row((2, 3, 32, 48), 64, 3, 1, 1, True) == nothing                                   # W % 32
    assert row((2, 3, 33, 32), 64, 3, 1, 1, True) == soft                                      # (H is free)
    assert row((2, 4, 32, 32), 64, 3, 1, 1, True) == nothing                                   # 3 input channels
    assert row((2, 3, 32, 32), 64, 3, 1, 0, True) == nothing
    assert row((2, 32, 32, 3), 64, 3, 1, 1, False) == ('conv_gemm_fwd', 'conv_wino_dgrad', 'conv_wgrad', '')     # an NCHW image
    # an epilogue takes the forward off the first-layer kernel, not the weight gradient, and the shape stays a first-layer shape
    assert row((2, 3, 32, 32), 64, 3, 1, 1, True, relu=True) == ('conv_gemm_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_onepass')
    assert row((2, 3, 32, 32), 64, 3, 1, 1, True, lrelu=True) == ('conv_gemm_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_onepass')


# ------------------------------------------------------------------------------------------------ switches, one at a time
HEADLINE = DARKCAPS['headline 416 x 416, batch 32 (BASELINE configs[2])'][2]
F22_ALL = [CONV1, F22, F22S2, F22S2, F22S2]
DIRECT = [CONV1, ('conv_gemm_fwd', 'conv_gemm_dgrad', 'conv_wgrad', 'dgrad_bn_fuse')] + [GEMM] * 3
S2_DGRAD_OFF = ('conv_wino42_fwd', 'conv_gemm_dgrad', 'conv_wino2_wgrad', 'in_affine dgrad_bn_fuse')
GENERIC1 = ('conv_gemm_fwd', None, 'conv_wgrad', '')
# switch off -> conv_1 .. conv_5 of the headline configuration (entries that keep their default row are written as HEADLINE[i])
SWITCH_OFF = {
    'USE_WINOGRAD': DIRECT,
    'USE_WINOGRAD4': [CONV1, ('conv_wino_fwd', 'conv_wino_dgrad', 'conv_wino4_wgrad', 'wgrad_bn wgrad_bn4')] + HEADLINE[2:],
    'USE_WINOGRAD4_WGRAD': [CONV1, F43_F22W] + HEADLINE[2:],
    'USE_WINOGRAD_S2': [CONV1, F43] + [GEMM] * 3,
    'USE_WINOGRAD_S2_DGRAD': [CONV1, F43] + [S2_DGRAD_OFF] * 3,
    'USE_WINOGRAD4_S2': [CONV1, F43] + [F22S2] * 3,
    'USE_WINOGRAD4_S2_DGRAD': [CONV1, F43] + [('conv_wino42_fwd', 'conv_wino2_dgrad', 'conv_wino2_wgrad', 'in_affine dgrad_bn_fuse dgrad_premasks')] * 3,
    'USE_CONV1': [GENERIC1] + HEADLINE[1:],
    'USE_CONV1_BWD': [('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_onepass')] + HEADLINE[1:],
    'USE_CONV1_MOMENTS': [('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_onepass')] + HEADLINE[1:],
    'USE_CONV1_ONEPASS': [('conv1_fwd', None, 'conv1_wgrad', 'conv1 conv1_bwd conv1_moments')] + HEADLINE[1:],
    'FUSE_BN_BWD_REDUCE': [CONV1, F43] + [('conv_wino42_fwd', 'conv_wino42_dgrad', 'conv_wino2_wgrad', 'in_affine')] * 3,
    'FUSE_BN_BWD_APPLY': [CONV1, ('conv_wino4_fwd', 'conv_wino4_dgrad', 'conv_wino4_wgrad', '')] + HEADLINE[2:],
}


@pytest.mark.parametrize('switch', SWITCHES)
def test_one_switch_off(switch, monkeypatch):
    """Exactly these entries of the headline configuration move, and the plan follows the switch at the next call (nothing cached)."""
    assert darkcaps_rows(416, 32) == HEADLINE
    monkeypatch.setattr(ops, switch, False)
    assert darkcaps_rows(416, 32) == SWITCH_OFF[switch]
    monkeypatch.setattr(ops, switch, True)
    assert darkcaps_rows(416, 32) == HEADLINE


def test_every_switch_is_covered():
    assert sorted(SWITCH_OFF) == sorted(SWITCHES)
    fp32_conv = [n for n in dir(ops) if n.startswith(('USE_', 'FUSE_')) and not n.endswith('_BF16') and n not in ('FUSE_POOL', 'FUSE_INPUT_AFFINE')]
    assert sorted(fp32_conv) == sorted(SWITCHES)        # (FUSE_POOL / FUSE_INPUT_AFFINE: whether FusedBackbone asks for a fusion at all)


# ------------------------------------------------------------------------------------------------ invariants over a grid
def grid():
    for (B, H, W), cin, cout, (k, s, p), nchw, epi in itertools.product(
            [(1, 6, 6), (2, 7, 8), (2, 32, 32), (3, 16, 48), (1, 512, 256), (2, 256, 256), (1, 512, 512), (1, 511, 512)],
            [3, 4, 8, 32, 64, 96, 128], [3, 8, 32, 64, 128], [(1, 1, 0), (3, 1, 1), (3, 1, 0), (3, 2, 1), (4, 2, 1), (4, 2, 0), (5, 1, 2)],
            [False, True], [{}, {'relu': True}, {'lrelu': True}]):
        yield ((B, cin, H, W) if nchw else (B, H, W, cin)), cout, k, s, p, nchw, epi


@pytest.mark.parametrize('off', [None] + list(SWITCHES))
def test_invariants(off, monkeypatch):
    if off is not None:
        monkeypatch.setattr(ops, off, False)
    n = 0
    for shape, cout, k, s, p, nchw, epi in grid():
        pl = ops.conv_plan(shape, cout, k, s, p, nchw, **epi)
        at = (off, shape, cout, k, s, p, nchw, epi, pl)
        if pl.in_affine:       # a fused input affine: forward AND weight gradient on a 4x4 / stride-2 Winograd family
            assert pl.fwd in ('conv_wino2_fwd', 'conv_wino42_fwd') and pl.wgrad == 'conv_wino2_wgrad', at
        if pl.dgrad_bn_fuse:   # the producer's BatchNorm-backward sums never ride a 3x3 Winograd input gradient
            assert pl.dgrad in ('conv_gemm_dgrad', 'conv_wino2_dgrad', 'conv_wino42_dgrad'), at
        if pl.dgrad_premasks:  # premasking only with the fused sums, only from the 4x4 / stride-2 Winograd kernels
            assert pl.dgrad_bn_fuse and pl.dgrad in ('conv_wino2_dgrad', 'conv_wino42_dgrad'), at
        if pl.wgrad_bn4:
            assert pl.wgrad_bn and pl.wgrad == 'conv_wino4_wgrad', at
        if pl.wgrad_bn:        # the fused BatchNorm-apply form exists where a 3x3 Winograd weight gradient does
            assert pl.wgrad in ('conv_wino_wgrad', 'conv_wino4_wgrad'), at
        assert pl.conv1 == (pl.wgrad == 'conv1_wgrad') and (pl.fwd != 'conv1_fwd' or pl.conv1), at
        assert (not pl.conv1_bwd or pl.conv1) and (not pl.conv1_moments or pl.conv1_bwd) and (not pl.conv1_onepass or pl.conv1), at
        assert (pl.dgrad is None) == nchw, at
        assert pl.fwd in ('conv_wino4_fwd', 'conv_wino_fwd', 'conv_wino42_fwd', 'conv_wino2_fwd', 'conv1_fwd', 'conv_gemm_fwd'), at
        assert pl.dgrad in (None, 'conv_wino4_dgrad', 'conv_wino_dgrad', 'conv_wino42_dgrad', 'conv_wino2_dgrad', 'conv_gemm_dgrad'), at
        assert pl.wgrad in ('conv_wino4_wgrad', 'conv_wino_wgrad', 'conv_wino2_wgrad', 'conv1_wgrad', 'conv_wgrad'), at
        n += 1
    assert n == 8 * 7 * 5 * 7 * 2 * 3


def test_plan_is_immutable():
    pl = ops.conv_plan((2, 32, 32, 64), 64, 3, 1, 1)
    with pytest.raises(AttributeError):
        pl.fwd = 'conv_gemm_fwd'

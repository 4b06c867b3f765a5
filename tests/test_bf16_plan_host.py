"""The bf16 GEMM's launch plan (csrc/conv_bf16.hip make_plan, exported as cy_conv_gemm_bf16_plan): which block tile, which K order
(TAPIN: taps inside a channel chunk), how many tiles and persistent blocks every launch of DarkCapsuleNet's bf16 backbone gets.
Host arithmetic: no GPU.  The headline rows (608 x 608, batch 32) are pinned literally; a change of any of them is a change of which
kernel runs the BASELINE configuration and has to be made here on purpose."""
import ctypes as C

import pytest

from helpers import REPO  # noqa: F401  (puts the repository on sys.path)

from capsyolo_amd import _lib, ops

# layer: (Cin, Cout, k, stride, input size as a fraction of the image) -- models.py _darkcaps_backbone behind the first block
LAYERS = {'conv_2': (128, 256, 3, 1, 1), 'conv_3': (256, 64, 4, 2, 1), 'conv_4': (64, 128, 4, 2, 2), 'conv_5': (128, 256, 4, 2, 4)}


def layer_plans(name, op, H, B, bnf=False):
    Cin, Cout, k, s, div = LAYERS[name]
    return ops.conv_bf16_plans(op, (B, H // div, H // div, Cin), Cout, k, s, 1, False, bnf)


def plan_tuple(p):
    return (p['BM'], p['BN'], p['TAPIN'], p['ntiles'], p['blocks'])


# (layer, op, fused BatchNorm-backward sums) -> (BM, BN, TAPIN, ntiles, blocks) at 608 x 608, batch 32 / batch 2, and at 96 x 96, batch 8
HEADLINE = [
    (('conv_2', 'fwd', False), (256, 256, 0, 46208, 256), (256, 256, 0, 2888, 256), (256, 256, 0, 288, 256)),
    (('conv_3', 'fwd', False), (512, 64, 1, 5776, 256), (512, 64, 1, 361, 256), (128, 64, 0, 144, 144)),
    (('conv_4', 'fwd', False), (512, 128, 0, 1444, 256), (512, 128, 0, 91, 91), (512, 128, 0, 9, 9)),
    (('conv_5', 'fwd', False), (256, 256, 0, 722, 256), (256, 256, 0, 46, 46), (256, 256, 0, 5, 5)),
    (('conv_2', 'dgrad', False), (512, 128, 1, 23104, 256), (512, 128, 1, 1444, 256), (512, 128, 1, 144, 144)),
    (('conv_3', 'dgrad', True), (256, 256, 0, 46208, 256), (256, 256, 0, 2888, 256), (256, 256, 0, 288, 256)),
    (('conv_4', 'dgrad', True), (512, 64, 1, 5776, 256), (128, 64, 0, 1444, 512), (128, 64, 0, 144, 144)),
    (('conv_5', 'dgrad', True), (512, 128, 1, 1444, 256), (512, 128, 1, 92, 92), (512, 128, 1, 12, 12)),
]


@pytest.mark.parametrize('row', HEADLINE, ids=['%s-%s' % r[0][:2] for r in HEADLINE])
def test_headline_layers_keep_their_plan(row):
    (name, op, bnf), b32, b2, small = row
    for (H, B), want in (((608, 32), b32), ((608, 2), b2), ((96, 8), small)):
        got = layer_plans(name, op, H, B, bnf)
        assert len(got) == 1, (name, op, H, B, got)            # the strided input gradients: the four parity classes in ONE launch
        assert plan_tuple(got[0]) == want, (name, op, H, B, got[0], want)


def desc(M_rows, Cin, N, taps=9, B=1):
    """A stride-1 forward of M_rows x 1 output pixels per image (the plan reads shapes only)."""
    k = 3 if taps == 9 else 1
    return ops._gemm_fwd_desc(*ops._x_geometry((B, M_rows, 1, Cin), False), N, k, 1, k // 2)


def plan_of(a, ncls=1, out_f32=0):
    p = (C.c_int * 5)()
    arr = (_lib.ConvGemm * ncls)(*([a] * ncls))
    rc = _lib.query('cy_conv_gemm_bf16_plan', arr, ncls, out_f32, p)
    return rc, tuple(p)


def test_plan_boundaries():
    # N = 64: the 512 x 64 tile from M = 512 * 256 output pixels on
    assert plan_of(desc(131071, 64, 64))[1][:3] == (128, 64, 0)
    assert plan_of(desc(131072, 64, 64))[1][:3] == (512, 64, 0)
    assert plan_of(desc(131072, 64, 192))[1][:3] == (512, 64, 0)
    # TAPIN from (Cin / 64) * BM > 768 on (and only with more than one tap)
    assert plan_of(desc(1000, 192, 256))[1][:3] == (256, 256, 0)                  # 3 * 256 = 768
    assert plan_of(desc(1000, 256, 256))[1][:3] == (256, 256, 1)
    assert plan_of(desc(1000, 384, 64))[1][:3] == (128, 64, 0)                    # 6 * 128 = 768
    assert plan_of(desc(1000, 448, 64))[1][:3] == (128, 64, 1)
    assert plan_of(desc(1000, 64, 128))[1][:3] == (512, 128, 0)                   # 1 * 512
    assert plan_of(desc(1000, 128, 128))[1][:3] == (512, 128, 1)
    assert plan_of(desc(1000, 1024, 256, taps=1))[1][:3] == (256, 256, 0)         # one tap: nothing to put inside
    # persistent blocks: min(ntiles, resident) with 256 resident 8-wave blocks and 512 of 128 x 64
    assert plan_of(desc(256 * 256, 64, 256))[1][3:] == (256, 256)
    assert plan_of(desc(256 * 256 + 1, 64, 256))[1][3:] == (257, 256)
    assert plan_of(desc(512 * 128, 64, 64))[1][3:] == (512, 512)
    assert plan_of(desc(512 * 128 + 1, 64, 64))[1][3:] == (513, 512)
    assert plan_of(desc(512 * 256 + 1, 64, 64))[1][2:] == (0, 257, 256)
    # parity classes multiply the tiles; the output type does not change the plan
    assert plan_of(desc(1000, 64, 64), ncls=4)[1][3:] == (32, 32)
    assert plan_of(desc(5000, 128, 128), out_f32=1)[1] == plan_of(desc(5000, 128, 128))[1]


def test_plan_refuses_what_the_launch_refuses():
    assert plan_of(desc(100, 96, 64))[0] != 0                                     # Cin not a multiple of 64
    assert plan_of(desc(100, 64, 64), ncls=5)[0] != 0
    a = desc(100, 64, 64)
    a.bn_red = 1
    assert plan_of(a, out_f32=1)[0] != 0                                          # fused sums need the bf16 output
    assert plan_of(a)[0] == 0
    assert plan_of(desc(1 << 20, 64, 64, B=1 << 11))[0] != 0                      # 2^31 output pixels
    assert b'2^31' in _lib.query('capsyolo_last_error')

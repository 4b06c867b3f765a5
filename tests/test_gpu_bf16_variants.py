"""Every compiled instantiation of the bf16 implicit-GEMM kernel (csrc/conv_bf16.hip: 4 block tiles x TAPIN 0 / 1 x the bf16, bf16 +
fused BatchNorm-backward sums and fp32 outputs = 24 kernels) against an EXACT reference, at shapes where each persistent block walks
at least two tiles (one case with one tile more than the resident blocks), with a partial last M tile and several N tiles.

Integer-valued data: x, w, dz and z in {-2..2}, integer bias.  Every fp32 partial sum of the GEMM is then an integer below 2^24 in
magnitude (|sum| <= 4 K + 2 with K <= 4032 here), so the fp32 accumulator is exact in any order and equals the float64 reference:
bf16 outputs must be the reference rounded to bf16 bit for bit, fp32 outputs the reference itself.  The LeakyReLU epilogue and the
fused BatchNorm-backward epilogue use slope 1/8; the BatchNorm constants are powers of two (scale, invstd), integers (mean) and
half-integers (shift), so that y = z * scale + shift, d and xhat are exact too.  The statistics and BatchNorm sums are fp32 per lane
before their double atomics: held to 1e-6 of their abs-sums.  Every case runs twice and must be bit-identical.

The plan of every launch is asserted (cy_conv_gemm_bf16_plan) before any value is checked, and the census below checks on the CPU
that the cases reach all 24 kernels."""
import pytest
import torch
import torch.nn.functional as F

from helpers import REPO  # noqa: F401

from capsyolo_amd import ops

BF = torch.bfloat16
SLOPE = 0.125
TILES = ((256, 256), (512, 128), (512, 64), (128, 64))
RESIDENT = {(256, 256): 256, (512, 128): 256, (512, 64): 256, (128, 64): 512}

# op, variant, B, H, W, Cin, Cout, k, stride (pad 1) -> (BM, BN, TAPIN) of every launch.  'fwd' is conv_forward_bf16 with the
# statistics epilogue (LeakyReLU epilogue where TAPIN = 1), 'dgrad' conv_dgrad_bf16 (GEMM Cin = the layer's Cout, N = its Cin; 4 x 4 /
# stride 2 on even sizes: the four parity classes in one launch, on odd sizes one launch per class).
VARIANT_CASES = [
    ('fwd', 'bf16', 2, 81, 203, 64, 512, 3, 1, (256, 256, 0)),         # 129 M tiles x 2 N tiles, last M tile partial
    ('fwd', 'bf16', 2, 81, 203, 256, 512, 3, 1, (256, 256, 1)),
    ('fwd', 'bf16', 1, 97, 451, 64, 384, 3, 1, (512, 128, 0)),         # 86 x 3 tiles
    ('fwd', 'bf16', 1, 97, 451, 128, 384, 3, 1, (512, 128, 1)),
    ('fwd', 'bf16', 4, 64, 521, 64, 64, 3, 1, (512, 64, 0)),           # M = 133376: 261 tiles of 512 x 64
    ('fwd', 'bf16', 4, 64, 521, 128, 192, 3, 1, (512, 64, 1)),         # 261 x 3
    ('fwd', 'bf16', 2, 40, 820, 64, 64, 3, 1, (128, 64, 0)),           # 513 tiles = resident + 1, last one half full
    ('fwd', 'bf16', 2, 40, 820, 448, 64, 3, 1, (128, 64, 1)),
    ('fwd', 'bf16', 1, 100, 401, 64, 192, 3, 1, (128, 64, 0)),         # 314 x 3
    ('fwd', 'f32', 2, 81, 203, 64, 512, 3, 1, (256, 256, 0)),
    ('fwd', 'f32', 2, 81, 203, 256, 512, 3, 1, (256, 256, 1)),
    ('fwd', 'f32', 1, 97, 451, 64, 384, 3, 1, (512, 128, 0)),
    ('fwd', 'f32', 1, 97, 451, 128, 384, 3, 1, (512, 128, 1)),
    ('fwd', 'f32', 4, 64, 521, 64, 64, 3, 1, (512, 64, 0)),
    ('fwd', 'f32', 4, 64, 521, 128, 192, 3, 1, (512, 64, 1)),
    ('fwd', 'f32', 2, 40, 820, 64, 64, 3, 1, (128, 64, 0)),
    ('fwd', 'f32', 2, 40, 820, 448, 64, 3, 1, (128, 64, 1)),
    ('dgrad', 'bnf', 2, 90, 190, 512, 64, 4, 2, (256, 256, 0)),        # 34 x 2 tiles x 4 classes
    ('dgrad', 'bnf', 2, 90, 190, 512, 256, 4, 2, (256, 256, 1)),
    ('dgrad', 'bnf', 2, 120, 184, 384, 64, 4, 2, (512, 128, 0)),       # 22 x 3 x 4
    ('dgrad', 'bnf', 2, 120, 184, 384, 128, 4, 2, (512, 128, 1)),
    ('dgrad', 'bnf', 4, 128, 1042, 64, 64, 4, 2, (512, 64, 0)),        # 133376 pixels per class: 261 x 4
    ('dgrad', 'bnf', 4, 128, 1042, 64, 128, 4, 2, (512, 64, 1)),       # (conv_4's input gradient at batch 32)
    ('dgrad', 'bnf', 2, 120, 280, 64, 64, 4, 2, (128, 64, 0)),         # 132 x 4
    ('dgrad', 'bnf', 2, 120, 280, 64, 448, 4, 2, (128, 64, 1)),
    ('dgrad', 'f32', 2, 120, 280, 64, 64, 4, 2, (128, 64, 0)),
    ('dgrad', 'bf16', 2, 91, 181, 128, 256, 4, 2, (512, 128, 1)),      # odd sizes: one launch per parity class, each its own grid
    ('dgrad', 'bf16', 2, 81, 203, 512, 64, 3, 1, (256, 256, 0)),       # stride 1: one class, 9 taps
]


def case_id(c):
    return '%s-%s-B%d-%dx%d-%d-%d-k%ds%d' % c[:9]


def plans_of(case):
    op, var, B, H, W, Cin, Cout, k, s, _ = case
    return ops.conv_bf16_plans(op, (B, H, W, Cin), Cout, k, s, 1, var == 'f32', var == 'bnf')


def test_variant_census_reaches_every_kernel():
    """CPU: the cases select the plans they name, and together all 24 kernels; every (variant, tile) has a case of two rounds."""
    seen, rounds = set(), set()
    for c in VARIANT_CASES:
        var = c[1]
        for p in plans_of(c):
            assert (p['BM'], p['BN'], p['TAPIN']) == c[9], (case_id(c), p)
            seen.add((var, p['BM'], p['BN'], p['TAPIN']))
            if p['ntiles'] > p['blocks']:
                rounds.add((var, p['BM'], p['BN']))
    want = set((v, bm, bn, t) for v in ('bf16', 'f32', 'bnf') for bm, bn in TILES for t in (0, 1))
    assert seen == want, sorted(want - seen)
    assert rounds >= set((v, bm, bn) for v in ('bf16', 'f32', 'bnf') for bm, bn in TILES), rounds
    assert any(p['ntiles'] == RESIDENT[(p['BM'], p['BN'])] + 1 for c in VARIANT_CASES for p in plans_of(c))


def ints(shape, gen, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=gen, device='cuda', dtype=torch.int8).to(BF)


def pow2(n, gen, lo=-1, hi=1):
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=gen, device='cuda').float())


def conv_ref(x, w, bias, s):
    """float64 conv on the GPU (exact for these integer values), NHWC in and out, chunked over the batch."""
    outs = []
    for b in range(x.shape[0]):
        outs.append(F.conv2d(x[b:b + 1].permute(0, 3, 1, 2).double(), w.double(), None if bias is None else bias.double(),
                             stride=s, padding=1).permute(0, 2, 3, 1))
    return torch.cat(outs)


def dgrad_ref(dz, w, in_shape, s):
    B, H, W, Cin = in_shape
    outs = []
    for b in range(B):
        outs.append(torch.nn.grad.conv2d_input((1, Cin, H, W), w.double(), dz[b:b + 1].permute(0, 3, 1, 2).double(),
                                               stride=s, padding=1).permute(0, 2, 3, 1))
    return torch.cat(outs)


def close_sums(got, want, abs_sum, what):
    err = (got - want).abs()
    bound = 1e-6 * abs_sum + 1e-9
    assert bool((err <= bound).all()), (what, float((err / bound.clamp(min=1e-30)).max()))


def same_bits(a, b):
    """Two kernel outputs: the same bits."""
    return torch.equal(a.view(torch.int16) if a.dtype == BF else a.view(torch.int32),
                       b.view(torch.int16) if b.dtype == BF else b.view(torch.int32))


def ord16(t):
    """bf16 bits as integers in the order of the values (+0 and -0 both 0): differences count ulps."""
    i = t.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


def equal_bf(a, ref):
    """A bf16 kernel output against the reference rounded to bf16: bit for bit (a zero's sign aside)."""
    return torch.equal(ord16(a), ord16(ref.to(BF)))


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize('case', VARIANT_CASES, ids=[case_id(c) for c in VARIANT_CASES])
def test_bf16_gemm_variant_exact(case):
    op, var, B, H, W, Cin, Cout, k, s, want = case
    for p in plans_of(case):
        assert (p['BM'], p['BN'], p['TAPIN']) == want, p
    gen = torch.Generator(device='cuda').manual_seed(1000 + VARIANT_CASES.index(case))
    w = ints((Cout, Cin, k, k), gen).float()
    out_f32 = var == 'f32'
    Ho, Wo = (H + 2 - k) // s + 1, (W + 2 - k) // s + 1
    if op == 'fwd':
        x = ints((B, H, W, Cin), gen)
        bias = torch.randint(-3, 4, (Cout,), generator=gen, device='cuda').float()
        lrelu = SLOPE if want[2] else None
        ref = conv_ref(x, w, bias, s)
        res = []
        for rep in range(2):
            stats = torch.zeros(ops.STATS_COPIES, Cout, 2, dtype=torch.float64, device='cuda')
            z = ops.conv_forward_bf16(x, w, bias, k, s, 1, stats, lrelu=lrelu, out_f32=out_f32)
            res.append((z, stats.sum(0)))
        torch.cuda.synchronize()
        assert same_bits(res[0][0], res[1][0]), 'run to run'
        act = ref if lrelu is None else torch.where(ref > 0, ref, ref * SLOPE)
        z = res[0][0]
        if out_f32:
            assert torch.equal(z.double(), act), float((z.double() - act).abs().max())
        else:
            assert equal_bf(z, act), int((ord16(z) != ord16(act.to(BF))).sum())
        r2 = ref.reshape(-1, Cout)
        for st in (res[0][1], res[1][1]):          # the statistics: of the fp32 accumulator plus bias, before the activation
            close_sums(st[:, 0], r2.sum(0), r2.abs().sum(0), 'sum')
            close_sums(st[:, 1], (r2 * r2).sum(0), (r2 * r2).sum(0), 'sum of squares')
        return
    dz = ints((B, Ho, Wo, Cout), gen)
    ref = dgrad_ref(dz, w, (B, H, W, Cin), s)
    if var != 'bnf':
        outs = [ops.conv_dgrad_bf16(dz, w, (B, H, W, Cin), k, s, 1, out_f32) for _ in range(2)]
        torch.cuda.synchronize()
        assert same_bits(outs[0], outs[1]), 'run to run'
        if out_f32:
            assert torch.equal(outs[0].double(), ref), float((outs[0].double() - ref).abs().max())
        else:
            assert equal_bf(outs[0], ref), int((ord16(outs[0]) != ord16(ref.to(BF))).sum())
        return
    z = ints((B, H, W, Cin), gen)
    sc, isd = pow2(Cin, gen), pow2(Cin, gen)
    sh = torch.randint(-2, 2, (Cin,), generator=gen, device='cuda').float() + 0.5
    mu = torch.randint(-1, 2, (Cin,), generator=gen, device='cuda').float()
    outs = []
    for rep in range(2):
        red = torch.zeros(ops.STATS_COPIES, Cin, 2, dtype=torch.float64, device='cuda')
        d = ops.conv_dgrad_bf16(dz, w, (B, H, W, Cin), k, s, 1, False, 'variant', (z, sc, sh, mu, isd, SLOPE, red))
        outs.append((d, red.sum(0)))
    torch.cuda.synchronize()
    assert same_bits(outs[0][0], outs[1][0]), 'run to run'
    y = z.double() * sc.double() + sh.double()
    dref = torch.where(y > 0, ref, ref * SLOPE).to(BF)
    assert equal_bf(outs[0][0], dref), int((ord16(outs[0][0]) != ord16(dref)).sum())
    dr = dref.double().reshape(-1, Cin)
    xh = ((z.double() - mu.double()) * isd.double()).reshape(-1, Cin)
    for red in (outs[0][1], outs[1][1]):
        close_sums(red[:, 0], dr.sum(0), dr.abs().sum(0), 'sum d')
        close_sums(red[:, 1], (dr * xh).sum(0), (dr * xh).abs().sum(0), 'sum d xhat')


# ------------------------------------------------------------------------------------------------ the batch-32 608 x 608 shapes
# The bf16 configuration (DarkCapsuleNet at 608 x 608, batch 32) is the only one with tensors of more than 2^31 elements: conv_2's
# output, its activation and their gradients hold 32 * 608^2 * 256 = 3.03e9.  Each op runs once at batch 32 on integer-valued data and
# again on the same images in smaller batches that get the SAME plan (tile, TAPIN, blocks; asserted): every output image must be bit
# for bit what the small batch gave (a GEMM row's K order depends on the plan only), images 11 and 22 straddle 2^31 bytes and 2^31
# elements of the big tensors.  The sums are held to 1e-6 of their abs-sums.  Peak memory about 25 GB.
HW = 608


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def big_ints(shape, seed):
    """Integer-valued bf16 tensor in {-2..2}, filled image by image (no int8 temporary of the whole tensor)."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.empty(shape, dtype=BF, device='cuda')
    for b in range(shape[0]):
        t[b] = ints(shape[1:], gen)
    return t


def same_plan(op, in_shape, Cout, k, s, B_small, bnf=False):
    big = ops.conv_bf16_plans(op, in_shape, Cout, k, s, 1, False, bnf)
    small = ops.conv_bf16_plans(op, (B_small,) + tuple(in_shape[1:]), Cout, k, s, 1, False, bnf)
    key = lambda ps: [(p['BM'], p['BN'], p['TAPIN'], p['blocks']) for p in ps]
    assert key(big) == key(small), (big, small)
    return big[0]


def chunks(B, b):
    """Batches of b images covering 0 .. B-1 (the last one may overlap its predecessor)."""
    out = [(i, i + b) for i in range(0, B - b + 1, b)]
    if out[-1][1] < B:
        out.append((B - b, B))
    return out


def band_ref(x_img, w, bias, r0, r1):
    """float64 rows r0 .. r1-1 of a 3 x 3 / stride 1 / pad 1 conv of one NHWC image."""
    H = x_img.shape[0]
    xs = x_img[max(r0 - 1, 0):min(r1 + 1, H)].permute(2, 0, 1)[None].double()
    xs = F.pad(xs, (1, 1, 1 if r0 == 0 else 0, 1 if r1 == H else 0))
    return F.conv2d(xs, w.double(), bias.double())[0].permute(1, 2, 0)


@pytest.mark.gpu
def test_batch32_conv2_and_conv3_forward_with_statistics():
    B = 32
    gen = torch.Generator(device='cuda').manual_seed(7)
    x = big_ints((B, HW, HW, 128), 8)
    w = ints((256, 128, 3, 3), gen).float()
    bias = torch.randint(-3, 4, (256,), generator=gen, device='cuda').float()
    p = same_plan('fwd', (B, HW, HW, 128), 256, 3, 1, 1)
    assert (p['BM'], p['BN'], p['TAPIN']) == (256, 256, 0)
    stats = torch.zeros(ops.STATS_COPIES, 256, 2, dtype=torch.float64, device='cuda')
    z = ops.conv_forward_bf16(x, w, bias, 3, 1, 1, stats)
    assert z.numel() > 2 ** 31
    want = torch.zeros(256, 2, dtype=torch.float64, device='cuda')
    absum = torch.zeros(256, dtype=torch.float64, device='cuda')
    for b in range(B):
        st = torch.zeros(ops.STATS_COPIES, 256, 2, dtype=torch.float64, device='cuda')
        zb = ops.conv_forward_bf16(x[b:b + 1], w, bias, 3, 1, 1, st)
        assert same_bits(z[b:b + 1], zb), b
        want += st.sum(0)
        absum += z[b].double().abs().sum(dim=(0, 1))
    close_sums(stats.sum(0)[:, 0], want[:, 0], absum * 1.01, 'conv_2 sum')
    close_sums(stats.sum(0)[:, 1], want[:, 1], want[:, 1], 'conv_2 sum of squares')
    for r0 in (0, 200, 424, HW - 16):          # image 31 against float64: top and bottom 16 rows, two interior bands
        ref = band_ref(x[B - 1], w, bias, r0, r0 + 16)
        assert equal_bf(z[B - 1, r0:r0 + 16], ref), r0
    del x, z
    free()
    # conv_3's forward READS a 3.03e9-element tensor (integer-valued again, so that image 31 can be held to float64)
    z = big_ints((B, HW, HW, 256), 9)
    w3 = ints((64, 256, 4, 4), gen).float()
    b3 = torch.randint(-3, 4, (64,), generator=gen, device='cuda').float()
    p = same_plan('fwd', (B, HW, HW, 256), 64, 4, 2, 2)
    assert (p['BM'], p['BN'], p['TAPIN']) == (512, 64, 1)
    stats = torch.zeros(ops.STATS_COPIES, 64, 2, dtype=torch.float64, device='cuda')
    z3 = ops.conv_forward_bf16(z, w3, b3, 4, 2, 1, stats)
    want = torch.zeros(64, 2, dtype=torch.float64, device='cuda')
    for i, j in chunks(B, 2):
        st = torch.zeros(ops.STATS_COPIES, 64, 2, dtype=torch.float64, device='cuda')
        assert same_bits(z3[i:j], ops.conv_forward_bf16(z[i:j], w3, b3, 4, 2, 1, st)), i
        want += st.sum(0)
    # (conv_3's |z| <= 4 * 4096 + 3: the bf16 output is exact to 1/128 -- abs-sum from it)
    absum = z3.double().abs().sum(dim=(0, 1, 2)) * 1.01
    close_sums(stats.sum(0)[:, 0], want[:, 0], absum, 'conv_3 sum')
    close_sums(stats.sum(0)[:, 1], want[:, 1], want[:, 1], 'conv_3 sum of squares')
    ref = conv_ref(z[B - 1:B, :20], w3, b3, 2)[0, :9]          # image 31's first output rows (their taps stay inside the first 20 rows)
    assert equal_bf(z3[B - 1, :9], ref)
    del z, z3
    free()


@pytest.mark.gpu
def test_batch32_input_gradients():
    """conv_2's input gradient (its dz has 3.03e9 elements) and conv_3's / conv_4's with the fused BatchNorm-backward sums (conv_3's
    writes d over the 3.03e9-element tensor and reads conv_2's z of the same size)."""
    B = 32
    gen = torch.Generator(device='cuda').manual_seed(17)
    w2 = ints((256, 128, 3, 3), gen).float()
    dz = big_ints((B, HW, HW, 256), 18)
    p = same_plan('dgrad', (B, HW, HW, 128), 256, 3, 1, 1)
    assert (p['BM'], p['BN'], p['TAPIN']) == (512, 128, 1)
    dx = ops.conv_dgrad_bf16(dz, w2, (B, HW, HW, 128), 3, 1, 1)
    for b in range(B):
        assert same_bits(dx[b:b + 1], ops.conv_dgrad_bf16(dz[b:b + 1], w2, (1, HW, HW, 128), 3, 1, 1)), b
    ref = dgrad_ref(dz[B - 1:B, :24], w2, (1, 24, HW, 128), 1)[0, :16]    # image 31's first 16 rows (the 24-row crop's pad is below them)
    assert equal_bf(dx[B - 1, :16], ref)
    del dz, dx
    free()
    for name, Cin, Cout, H, b_small, tile in (('conv_3', 256, 64, HW, 1, (256, 256, 0)), ('conv_4', 64, 128, HW // 2, 6, (512, 64, 1))):
        w = ints((Cout, Cin, 4, 4), gen).float()
        dzl = ints((B, H // 2, H // 2, Cout), gen)
        z = big_ints((B, H, H, Cin), 19)
        sc, isd = pow2(Cin, gen), pow2(Cin, gen)
        sh = torch.randint(-2, 2, (Cin,), generator=gen, device='cuda').float() + 0.5
        mu = torch.randint(-1, 2, (Cin,), generator=gen, device='cuda').float()
        p = same_plan('dgrad', (B, H, H, Cin), Cout, 4, 2, b_small, bnf=True)
        assert (p['BM'], p['BN'], p['TAPIN']) == tile, name
        red = torch.zeros(ops.STATS_COPIES, Cin, 2, dtype=torch.float64, device='cuda')
        d = ops.conv_dgrad_bf16(dzl, w, (B, H, H, Cin), 4, 2, 1, False, name, (z, sc, sh, mu, isd, SLOPE, red))
        for i, j in chunks(B, b_small):
            r1 = torch.zeros(ops.STATS_COPIES, Cin, 2, dtype=torch.float64, device='cuda')
            dj = ops.conv_dgrad_bf16(dzl[i:j], w, (j - i, H, H, Cin), 4, 2, 1, False, name, (z[i:j], sc, sh, mu, isd, SLOPE, r1))
            assert same_bits(d[i:j], dj), (name, i)
        s1 = torch.zeros(Cin, dtype=torch.float64, device='cuda'); s2 = torch.zeros_like(s1)
        a1 = torch.zeros_like(s1); a2 = torch.zeros_like(s1)
        for b in range(B):                  # the sums of the stored (bf16) d, in float64
            db, xh = d[b].double().reshape(-1, Cin), ((z[b].double() - mu.double()) * isd.double()).reshape(-1, Cin)
            s1 += db.sum(0); a1 += db.abs().sum(0); s2 += (db * xh).sum(0); a2 += (db * xh).abs().sum(0)
            del db, xh
        close_sums(red.sum(0)[:, 0], s1, a1, name + ' sum d')
        close_sums(red.sum(0)[:, 1], s2, a2, name + ' sum d xhat')
        ref = dgrad_ref(dzl[B - 1:B, :12], w, (1, 24, H, Cin), 2)[0, :16]     # image 31's first 16 rows against float64
        y = z[B - 1, :16].double() * sc.double() + sh.double()
        assert equal_bf(d[B - 1, :16], torch.where(y > 0, ref, ref * SLOPE)), name
        del z, d
        free()


@pytest.mark.gpu
def test_batch32_conv2_weight_gradient_plain_and_fused():
    """conv_2's weight gradient at batch 32 (X 1.5e9, dZ / D / Z / the written dZ 3.03e9 elements) against the sum of the per-image
    weight gradients at 1e-5 relative L2; the fused kernel's written dZ bit-identical image by image."""
    from capsyolo_amd._lib import call, query
    B = 32
    gen = torch.Generator(device='cuda').manual_seed(27)
    st = torch.cuda.current_stream().cuda_stream
    x = big_ints((B, HW, HW, 128), 28)
    d = big_ints((B, HW, HW, 256), 29)
    dW = ops.conv_wgrad_bf16(x, d, 3, 1, 1)
    want = torch.zeros_like(dW, dtype=torch.float64)
    for b in range(B):
        want += ops.conv_wgrad_bf16(x[b:b + 1], d[b:b + 1], 3, 1, 1).double()
    assert rel_l2(dW, want) < 1e-5, rel_l2(dW, want)
    z = big_ints((B, HW, HW, 256), 30)
    sc, isd = pow2(256, gen), pow2(256, gen)
    mu = torch.randint(-1, 2, (256,), generator=gen, device='cuda').float()
    P = B * HW * HW
    red = (torch.randint(-1000, 1001, (256, 2), generator=gen, device='cuda').double() * (P / 1024))
    dz = torch.empty_like(z)
    nws = query('cy_conv_wgrad_bf16_bn_ws_floats', B, HW, HW, 128, 256, 3, 1)
    dWf = torch.empty(256, 128, 3, 3, device='cuda'); ws = torch.empty(nws, device='cuda')
    call('cy_conv_wgrad_bf16_bn', x.data_ptr(), d.data_ptr(), z.data_ptr(), dz.data_ptr(), dWf.data_ptr(), ws.data_ptr(), sc.data_ptr(),
         mu.data_ptr(), isd.data_ptr(), red.data_ptr(), None, None, B, HW, HW, 128, HW, HW, 256, 3, 1, st)
    del ws
    want = torch.zeros_like(dWf, dtype=torch.float64)
    red1 = red / B                                        # the same means per image (B a power of two: exact)
    nws1 = query('cy_conv_wgrad_bf16_bn_ws_floats', 1, HW, HW, 128, 256, 3, 1)
    for b in range(B):
        dz1 = torch.empty_like(z[b:b + 1]); dW1 = torch.empty_like(dWf); ws1 = torch.empty(nws1, device='cuda')
        call('cy_conv_wgrad_bf16_bn', x[b].data_ptr(), d[b].data_ptr(), z[b].data_ptr(), dz1.data_ptr(), dW1.data_ptr(), ws1.data_ptr(),
             sc.data_ptr(), mu.data_ptr(), isd.data_ptr(), red1.data_ptr(), None, None, 1, HW, HW, 128, HW, HW, 256, 3, 1, st)
        assert same_bits(dz[b:b + 1], dz1), b
        want += dW1.double()
    assert rel_l2(dWf, want) < 1e-5, rel_l2(dWf, want)
    del x, d, z, dz
    free()


@pytest.mark.gpu
def test_batch32_bn_act_kernels_on_the_largest_tensor():
    """cy_affine_act_bf16, cy_bn_bwd_reduce_bf16 and cy_bn_bwd_apply_bf16 over conv_2's 3.03e9-element output: the last image within
    one bf16 ulp of a float64 restatement, the sums at 1e-6 of their abs-sums."""
    from capsyolo_amd._lib import call
    B, N = 32, 256
    P = B * HW * HW
    gen = torch.Generator(device='cuda').manual_seed(37)
    st = torch.cuda.current_stream().cuda_stream
    z = big_ints((B, HW, HW, N), 38)
    sc, isd = pow2(N, gen), pow2(N, gen)
    sh = torch.randint(-2, 2, (N,), generator=gen, device='cuda').float() + 0.5
    mu = torch.randint(-1, 2, (N,), generator=gen, device='cuda').float()
    scd, shd, mud, isdd = sc.double(), sh.double(), mu.double(), isd.double()
    a = torch.empty_like(z)
    call('cy_affine_act_bf16', z.data_ptr(), a.data_ptr(), sc.data_ptr(), sh.data_ptr(), SLOPE, P, N, 0, st)
    y = z[B - 1].double() * scd + shd
    ulps = lambda u, v: int((ord16(u) - ord16(v.to(BF))).abs().max())
    assert ulps(a[B - 1], torch.where(y > 0, y, y * SLOPE)) <= 1
    da = a                                                 # (any bf16 gradient: the activation tensor itself)
    red = torch.empty(N, 2, dtype=torch.float64, device='cuda')
    call('cy_bn_bwd_reduce_bf16', z.data_ptr(), da.data_ptr(), 0, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), isd.data_ptr(), SLOPE,
         red.data_ptr(), P, N, st)
    s = [torch.zeros(N, dtype=torch.float64, device='cuda') for _ in range(4)]
    for b in range(B):
        zb = z[b].double().reshape(-1, N)
        db = torch.where(zb * scd + shd > 0, 1.0, SLOPE).double() * da[b].double().reshape(-1, N)
        xh = (zb - mud) * isdd
        s[0] += db.sum(0); s[1] += db.abs().sum(0); s[2] += (db * xh).sum(0); s[3] += (db * xh).abs().sum(0)
        del zb, db, xh
    close_sums(red[:, 0], s[0], s[1], 'sum d')
    close_sums(red[:, 1], s[2], s[3], 'sum d xhat')
    # the apply on sums of dyadic means (m1, m2 in eighths): every intermediate is then exact up to the last fp32 rounding
    redd = torch.randint(-16, 17, (N, 2), generator=gen, device='cuda').double() / 8 * P
    dz = torch.empty_like(z)
    dg, dbeta = torch.empty(N, device='cuda'), torch.empty(N, device='cuda')
    call('cy_bn_bwd_apply_bf16', z.data_ptr(), da.data_ptr(), 0, dz.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), isd.data_ptr(),
         SLOPE, redd.data_ptr(), dg.data_ptr(), dbeta.data_ptr(), P, N, st)
    zb = z[B - 1].double()
    d64 = torch.where(zb * scd + shd > 0, 1.0, SLOPE).double() * da[B - 1].double()
    assert ulps(dz[B - 1], scd * (d64 - redd[:, 0] / P - (zb - mud) * isdd * (redd[:, 1] / P))) <= 1
    del z, a, dz
    free()

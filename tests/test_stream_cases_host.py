"""CPU tests of the streaming-kernel case table (tests/stream_cases.py): what makes tests/test_gpu_streaming.py mean something.
(a) every case keeps the conditions it was made for -- the margins with no element left out, the intended launch path, the loop counts,
restated from the launchers of csrc/bn.hip and csrc/misc.hip; (b) the numpy reference is the definition: it gives what torch's own
modules give in float64; (c) the reference alone passes: its float32 evaluation is accepted by `compare` on every case; (d) the cases
catch wrong kernels: mutants of the reference (float32, each a plausible kernel bug) are rejected, each on a case that is named."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_cases as S

T = torch.from_numpy
SMALL = S.names(big=False)
DOUBLE_INPUTS = ('stats', 'red', 'red_copies')


def _f32_representable(a):
    return a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------------------------------------ (a) the conditions
@pytest.mark.parametrize('name', S.names())
def test_inputs_are_float32_representable_float64(name):
    c = S.case(name)
    for k, v in c.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == 'f':
            assert v.dtype == np.float64, k
            if k not in DOUBLE_INPUTS:
                assert _f32_representable(v), k


def _argument(c):
    z = c['z']
    return z if c['scale'] is None else z * c['scale'] + c['shift']


@pytest.mark.parametrize('name', S.names('affine_act') + S.names('bn_bwd_reduce') + S.names('bn_bwd_apply'))
def test_every_activation_argument_is_away_from_zero(name):
    c = S.case(name)
    if c.get('exact'):                                                  # the dyadic case: halves, never 0, and exact in any arithmetic
        assert (_argument(c) != 0).all() and np.abs(_argument(c)).min() >= 0.5
        return
    y = _argument(c)
    assert y.shape == (c['P'], c['N']) and np.abs(y).min() >= S.MARGIN, np.abs(y).min()
    assert (y > 0).any() and (y < 0).any() or y.size < 4
    if c['scale'] is not None:
        assert (c['scale'] < 0).any() and c['scale'][0] < 0 and (c['scale'] != 0).all()
        if c['N'] > 1:                                                  # where z and the argument disagree in sign, in numbers
            assert ((c['z'] > 0) != (y > 0)).mean() > 0.05


@pytest.mark.parametrize('name', S.names('act_bwd'))
def test_act_bwd_zeros_take_the_slope_branch(name):
    c = S.case(name)
    z = c['z']
    others = np.ones(z.size, dtype=bool)
    others[c['zeros']] = False
    assert (z[c['zeros']] == 0).all() and np.signbit(z[c['zeros']]).any() and not np.signbit(z[c['zeros']]).all()
    assert np.abs(z[others]).min() >= S.MARGIN
    assert c['n'] % 256 != 0 and c['n'] > 256
    dz = S.reference(name)['dz']
    assert np.array_equal(dz[c['zeros']], c['da'][c['zeros']] * c['slope'])


@pytest.mark.parametrize('name', S.names('maxpool'))
def test_pooling_windows_have_a_clear_winner_or_a_hand_built_tie(name):
    c = S.case(name)
    x = c['x']
    B, H, W, C = x.shape
    assert c['path'] == ('vector' if C % 4 == 0 and not c['offset'] else 'scalar')
    if H // 2 == 0 or W // 2 == 0:
        assert S.reference(name)['y'].size == 0 and not S.reference(name)['dx'].any()
        return
    top = np.sort(S.windows(x), axis=0)
    gap = top[3] - top[2]
    if not c['ties']:
        assert gap.min() >= S.MARGIN
        return
    # the hand-built windows: a gap of 0 with equal values exactly where the table says so, a clear winner elsewhere
    assert int((gap[0, 0, :, 0] == 0).sum()) == c['ties'] == sum(1 for v, _ in S.TIE_WINDOWS if sorted(v)[-1] == sorted(v)[-2])
    assert (gap[gap != 0] >= S.MARGIN).all()
    ref = S.reference(name)
    for i, (v, winner) in enumerate(S.TIE_WINDOWS):
        for ch in range(C):
            assert ref['y'][0, 0, i, ch] == v[winner] and np.signbit(ref['y'][0, 0, i, ch]) == np.signbit(v[winner])
            got = [ref['dx'][0, 0, 2 * i, ch], ref['dx'][0, 0, 2 * i + 1, ch], ref['dx'][0, 1, 2 * i, ch], ref['dx'][0, 1, 2 * i + 1, ch]]
            assert [j for j in range(4) if got[j] != 0] == [winner]
    assert any(max(v) < 0 for v, _ in S.TIE_WINDOWS)                    # the all-negative window


def test_affine_act_cases_reach_every_launch_variant_with_a_tail():
    seen, Ns, slopes = set(), set(), set()
    for name in S.names('affine_act', big=False) + ['affine_act/hoist_affine_nt_over_128mib']:
        if name in S.BIG:                                               # the shape alone: the arrays are not needed here
            P, N = S.FACTORY[name].args[1:3]
            c = dict(P=P, N=N, scale=1, offset=False, path=S.FACTORY[name].args[4], slope=0.1)
        else:
            c = S.case(name)
        P, N = c['P'], c['N']
        path = S.affine_path(P, N, c['scale'] is not None, c['offset'])
        assert path == c['path'], name
        seen.add(path)
        Ns.add(N)
        slopes.add(c['slope'])
        if path.startswith('hoist'):
            n4 = P * N // 4
            ut = S.unrolled_and_tail(n4, S.stream_grid(n4) * 256, 4)
            assert any(u >= 1 for u, t in ut) and any(t >= 1 for u, t in ut), name      # the unrolled body and the tail loop both run
        else:
            n = P * N // 4 if path.startswith('vector') else P * N
            # more than one block, the last one partly empty (2048 channels: 512 float4 a row, no such size)
            assert n > 256 and (n % 256 != 0 or N == 2048), name
        if path == 'hoist_affine_nt':
            assert 33554432 < P * N < 33554432 + 1024
    assert seen == {'hoist_affine', 'hoist_affine_nt', 'hoist_plain', 'vector_affine', 'vector_plain', 'scalar'}
    assert Ns >= {4, 64, 1024, 12, 40, 2048, 10, 3} and slopes == {0.1, 0.0, 1.0}
    assert S.case('affine_act/scalar_n64_offset_view')['offset'] and S.affine_path(157, 64, True, False) == 'hoist_affine'


def test_reduce_cases_cover_the_slice_layouts_and_the_loop():
    Ns, slopes = set(), set()
    for name in S.names('bn_bwd_reduce', big=False):
        c = S.case(name)
        P, N = c['P'], c['N']
        rpar, rpb, blocks = S.reduce_plan(P, N)
        lpr = min(N, 64) // 4                                           # lanes per row; rows in parallel in a block of 256
        assert rpar == 256 // lpr and rpb % rpar == 0 and rpb >= 4 * rpar and blocks == S.ceil_div(P, rpb) * max(1, N // 64)
        assert P in (1, rpar - 1, 4 * rpar, 4 * rpar + 1)
        Ns.add(N)
        slopes.add(c['slope'])
    assert Ns == {4, 8, 32, 64, 128, 1024} and slopes == {0.1, 1.0, 0.0}
    for N in Ns:
        rpar = 256 // (min(N, 64) // 4)
        assert {S.case(n)['P'] for n in S.names('bn_bwd_reduce', big=False) if S.case(n)['N'] == N} == {1, rpar - 1, 4 * rpar, 4 * rpar + 1}
    assert S.reduce_plan(64, 1024)[2] == 16                             # 16 channel slices
    P, N = S.FACTORY['bn_bwd_reduce/n64_two_unrolled_and_tail'].args[2:4]
    rpar, rpb, blocks = S.reduce_plan(P, N)
    assert N == 64 and rpar == 16 and rpb >= 9 * rpar and blocks > 1 and P % rpb != 0
    assert (2, 2) in S.unrolled_and_tail(rpb, rpar, 4)                  # a thread of a full block: the unrolled body twice, then the tail
    for N in S.REFUSED_REDUCE_N:
        assert S.reduce_plan(100, N) is None


def test_apply_cases_reach_both_kernels_with_a_tail():
    Ns, grads = set(), set()
    for name in S.names('bn_bwd_apply'):
        c = S.case(name)
        assert S.apply_path(c['N']) == c['path'], name
        n4 = c['P'] * c['N'] // 4
        assert c['P'] * c['N'] % 4 == 0
        Ns.add(c['N'])
        grads.add(c['param_grads'])
        if c.get('exact'):
            continue
        if c['path'] == 'hoist':
            ut = S.unrolled_and_tail(n4, S.stream_grid(n4) * 256, 2)
            assert any(u >= 1 for u, t in ut) and any(t >= 1 for u, t in ut), name
        else:
            assert n4 > 256 and (n4 % 256 != 0 or c['N'] == 2048), name
    assert Ns >= {4, 256, 1024, 12, 40, 2048} and grads == {True, False}


def test_above_cap_cases_run_the_unrolled_body_twice_and_the_tail():
    for kind, need in (('affine_act', 9), ('bn_bwd_apply', 5)):
        a = S.ABOVE_CAP[kind]
        n4 = a['P'] * a['N'] // 4
        stride = S.STREAM_CAP * 256
        assert S.stream_grid(n4) == S.STREAM_CAP and n4 >= need * stride and n4 % stride != 0 and n4 < (need + 1) * stride
        assert any(u == 2 and t >= 1 for u, t in S.unrolled_and_tail(n4, stride, a['unroll']))
        assert 1024 % a['N'] == 0


def test_misc_cases_over_the_grid_cap_make_the_grid_loop():
    cap = S.MISC_CAP * 256
    assert cap == 2097152
    f = S.FACTORY
    B, H, W, C = f['maxpool/scalar_grid_loops'].args[1:5]
    assert C % 4 != 0 and B * (H // 2) * (W // 2) * C > cap
    B, H, W, C = f['maxpool/vector_grid_loops'].args[1:5]
    assert C % 4 == 0 and B * (H // 2) * (W // 2) * C // 4 > cap
    B, H, W, C, fac = f['upsample/over_the_grid_cap'].args[1:6]
    assert B * H * W * C > cap                                          # the backward's grid (input elements) and so the forward's
    assert int(np.prod(f['permute/nchw_to_nhwc_over_the_grid_cap'].args[2])) > cap
    assert S.misc_grid(cap + 1) == S.MISC_CAP


def test_small_case_sets():
    assert {S.case(n)['N'] for n in S.names('bn_finalize')} == {1, 3, 256, 257, 1024}
    assert {S.case(n)['momentum'] for n in S.names('bn_finalize')} == {0.1, 1.0}
    assert {S.case(n)['per_out'] for n in S.names('bn_fold')} == {1, 27, 48, 288}
    assert any(S.case(n)['bias'] is None for n in S.names('bn_fold'))
    assert any(S.case(n)['Cout'] * S.case(n)['per_out'] % 256 for n in S.names('bn_fold'))
    assert all((S.case(n)['gamma'] < 0).any() for n in S.names('bn_fold') + S.names('bn_eval'))
    cs = [S.case(n) for n in S.names('channel_sum')]
    assert {c['N'] for c in cs} == {1, 10, 64, 65, 200} and {c['P'] for c in cs} == {1, 63, 64, 65, 5000}
    for c in cs:
        if c['exact']:                                                  # small integers: every partial sum is a float32, in any order
            assert np.array_equal(c['dz'], np.round(c['dz'])) and np.abs(c['dz']).sum(0).max() < 2 ** 24
            assert np.array_equal(S.reference(c['name'])['out'], c['dz'].astype(np.int64).sum(0))
    assert {S.case(n)['copies'] for n in S.names('bn_red_fold')} == {1, S.COPIES}
    assert sorted(S.case(n)['outs'] for n in S.names('bn_red_fold') if not all(S.case(n)['outs']))[:3] == \
        [(False, True, True), (True, False, False), (True, False, True)]
    ups = [S.case(n) for n in S.names('upsample', big=False)]
    assert {c['f'] for c in ups} == {1, 2, 3} and {c['x'].shape[3] for c in ups} == {1, 6} and all(c['x'].shape[1] != c['x'].shape[2] for c in ups)
    x = S.case('tanh/range')['x']
    assert x.min() < -12 and x.max() > 12 and (x == 0).any() and (np.abs(x) == np.float64(np.float32(1e-8))).sum() == 2
    heads = [S.case(n) for n in S.names('yolo_head')]
    assert {(c['split'], c['C']) for c in heads} >= {(10, 43), (0, 5), (10, 0), (5, 1)} and any(c['cells'] % 256 for c in heads)
    assert np.abs(S.case('yolo_head/logits_80')['x']).max() == 80
    for n in S.names('pick'):
        c = S.case(n)
        assert c['y'].min() == 0 and c['y'].max() == c['caps'].shape[1] - 1     # labels 0 and C - 1, none out of range
    assert S.case('pick/d1')['caps'].shape[2] == 1
    perms = [S.case(n) for n in S.names('permute', big=False)]
    assert {c['op'] for c in perms} == {'nchw_to_nhwc', 'nhwc_to_nchw', 'primary_caps_rows'}


@pytest.mark.parametrize('name', S.names('bn_finalize'))
def test_finalize_cases_and_reference_against_batch_norm(name):
    c = S.case(name)
    N, count = c['N'], c['count']
    assert c['stats'].shape == (S.COPIES, N, 2)
    empty = (c['stats'] == 0).all(axis=(1, 2))
    assert empty.any() and (count == 1 or (~empty).sum() > 1 or 'clamp' in name)
    tot = c['stats'].sum(0)
    if N >= 3:
        assert c['gamma'][0] == 0 and c['gamma'][2] < 0
    ref = S.reference(name)
    assert ref['nbt'] == c['nbt'] + 1
    if 'clamp' in name:                                                 # the sums give a variance below zero: -2^-13 against eps = 1e-5
        raw = tot[1, 1] / count - (tot[1, 0] / count) ** 2
        assert raw < -c['eps'] and ref['invstd'][1] == 1.0 / np.sqrt(c['eps']) and ref['running_var'][1] == 0.9 * c['running_var'][1]
        keep = np.array([0, 2])
    else:
        keep = np.arange(N)
        assert np.allclose(tot[:, 0], c['x'].sum(0), rtol=1e-14, atol=1e-13) and np.allclose(tot[:, 1], (c['x'] ** 2).sum(0), rtol=1e-14)
    if count == 1:                                                      # the unbiased variance of one value: the biased one, 0
        assert np.array_equal(ref['running_var'], 0.9 * c['running_var']) and (ref['invstd'] == 1.0 / np.sqrt(c['eps'])).all()
        return
    rm = T(c['running_mean'].copy()) if c['running_mean'] is not None else None
    rv = T(c['running_var'].copy()) if c['running_var'] is not None else None
    x = T(c['x'].copy())
    out = F.batch_norm(x, rm, rv, T(c['gamma'].copy()), T(c['beta'].copy()), True, c['momentum'], c['eps']).numpy()
    mine = c['x'] * ref['scale'] + ref['shift']
    assert np.allclose(mine[:, keep], out[:, keep], rtol=1e-9, atol=1e-9)
    assert np.allclose(ref['mean'], c['x'].mean(0), rtol=1e-12, atol=1e-13)
    assert np.allclose(ref['invstd'][keep], 1.0 / np.sqrt(c['x'].var(0) + c['eps'])[keep], rtol=1e-9)
    if rm is not None:
        assert np.allclose(ref['running_mean'], rm.numpy(), rtol=1e-12, atol=1e-13)
        assert np.allclose(ref['running_var'], rv.numpy(), rtol=1e-9, atol=1e-12)
    else:
        assert 'running_mean' not in ref and 'running_var' not in ref


# ------------------------------------------------------------------------------------------------ (b) the reference is the definition
def _nchw(a):
    return T(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))


def _torch_pair(fn, x_nchw, g_nhwc):
    x = x_nchw.clone().requires_grad_(True)
    y = fn(x)
    y.backward(_nchw(g_nhwc))
    return y.detach().permute(0, 2, 3, 1).numpy(), x.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('name', S.names('maxpool', big=False))
def test_pool_reference_is_max_pool2d(name):
    c, ref = S.case(name), S.reference(name)
    if ref['y'].size == 0:
        return
    y, dx = _torch_pair(lambda x: F.max_pool2d(x, 2), _nchw(c['x']), c['g'])
    assert S._same_bits(ref['y'], y) and S._same_bits(ref['dx'], dx)


@pytest.mark.parametrize('name', S.names('upsample', big=False))
def test_upsample_reference_is_interpolate(name):
    c, ref = S.case(name), S.reference(name)
    y, dx = _torch_pair(lambda x: F.interpolate(x, scale_factor=c['f'], mode='nearest'), _nchw(c['x']), c['g'])
    assert S._same_bits(ref['y'], y) and S._same_bits(ref['dx'], dx)


@pytest.mark.parametrize('name', S.names('yolo_head') + S.names('tanh'))
def test_head_and_tanh_references_are_torch(name):
    c, ref = S.case(name), S.reference(name)
    x = T(c['x'].copy()).requires_grad_(True)
    if c['kind'] == 'tanh':
        y = torch.tanh(x)
    else:
        y = torch.cat((torch.sigmoid(x[:, :c['split']]), F.softmax(x[:, c['split']:], dim=-1)), dim=-1)
    y.backward(T(c['g'].copy()))
    assert np.allclose(ref['y'], y.detach().numpy(), rtol=1e-12, atol=1e-300) and np.isfinite(ref['y']).all()
    assert np.allclose(ref['dx'], x.grad.numpy(), rtol=1e-9, atol=1e-15) and np.isfinite(ref['dx']).all()
    if name == 'yolo_head/one_class':                                   # a softmax over one class: identically 1, gradient exactly 0
        assert (ref['y'][:, -1] == 1).all() and not ref['dx'][:, -1].any()
        r32 = S.reference(name, np.float32)
        assert (r32['y'][:, -1] == 1).all() and not r32['dx'][:, -1].any()


@pytest.mark.parametrize('name', S.names('permute', big=False) + S.names('pick'))
def test_permute_and_pick_references_are_torch(name):
    c, ref = S.case(name), S.reference(name)
    if c['kind'] == 'pick':
        caps = T(c['caps'].copy()).requires_grad_(True)
        out = caps.gather(1, T(c['y'])[:, None, None].expand(-1, 1, caps.shape[2])).squeeze(1)
        out.backward(T(c['g'].copy()))
        assert S._same_bits(ref['out'], out.detach().numpy()) and S._same_bits(ref['dcaps'], caps.grad.numpy())
        return
    x = T(c['x'].copy()).requires_grad_(True)
    if c['op'] == 'nchw_to_nhwc':
        y = x.permute(0, 2, 3, 1)
    elif c['op'] == 'nhwc_to_nchw':
        y = x.permute(0, 3, 1, 2)
    else:       # the n_caps convolutions of the primary capsules, each NCHW, flattened and concatenated on a new last axis
        B, H, W, Cc = x.shape
        per_cap = [x[..., cap::c['n_caps']].permute(0, 3, 1, 2) for cap in range(c['n_caps'])]
        y = torch.cat([t.reshape(B, -1, 1) for t in per_cap], dim=-1)
    y.contiguous().backward(T(c['g'].copy()))
    assert S._same_bits(ref['y'], y.detach().contiguous().numpy()) and S._same_bits(ref['dx'], x.grad.numpy())


def test_bn_backward_reference_is_autograd():
    """Reduce + apply on a block's own statistics give the gradient of LeakyReLU(BatchNorm2d(z)) by autograd, dgamma and dbeta too."""
    rng = np.random.default_rng(7)
    P, N, slope, eps = 50, 12, 0.1, 1e-5
    z, da = S.f32(rng.standard_normal((P, N)) + 0.3), S.f32(rng.standard_normal((P, N)))
    gamma, beta = S.f32(rng.uniform(0.5, 1.5, N) * np.where(np.arange(N) % 3 == 0, -1, 1)), S.f32(0.2 * rng.standard_normal(N))
    zt, gt, bt = (T(a.copy()).requires_grad_(True) for a in (z, gamma, beta))
    F.leaky_relu(F.batch_norm(zt, None, None, gt, bt, True, 0.1, eps), slope).backward(T(da.copy()))
    mean, invstd = z.mean(0), 1.0 / np.sqrt(z.var(0) + eps)
    c = dict(kind='bn_bwd_reduce', P=P, N=N, z=z, da=da, scale=gamma * invstd, shift=beta - mean * gamma * invstd, mean=mean, invstd=invstd,
             slope=slope)
    red = S.Ref().bn_bwd_reduce(c)['red']
    out = S.Ref().bn_bwd_apply(dict(c, red=red, param_grads=True))
    assert np.allclose(out['dz'], zt.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert np.allclose(out['dgamma'], gt.grad.numpy(), rtol=1e-9, atol=1e-12) and np.allclose(out['dbeta'], bt.grad.numpy(), rtol=1e-9, atol=1e-12)
    act = S.Ref().affine_act(dict(c, kind='affine_act'))['a']
    assert np.allclose(act, F.leaky_relu(F.batch_norm(T(z.copy()), None, None, T(gamma.copy()), T(beta.copy()), True, 0.1, eps), slope).numpy(),
                       rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('name', S.names('bn_fold'))
def test_fold_reference_is_eval_batch_norm_behind_the_convolution(name):
    c, ref = S.case(name), S.reference(name)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, c['per_out']))
    b = c['bias'] if c['bias'] is not None else 0.0
    want = F.batch_norm(T(x @ c['W'].T + b), T(c['running_mean'].copy()), T(c['running_var'].copy()), T(c['gamma'].copy()), T(c['beta'].copy()),
                        False, 0.1, c['eps']).numpy()
    assert np.allclose(x @ ref['Wf'].T + ref['bf'], want, rtol=1e-9, atol=1e-12)
    ev = S.Ref().bn_eval(c)
    assert np.allclose((x @ c['W'].T + b) * ev['scale'] + ev['shift'], want, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ (c) the reference alone passes
@pytest.mark.parametrize('name', S.names())
def test_reference_in_float32_passes(name):
    c = S.case(name)
    fr = S.compare(c, S.reference(name, np.float32))
    print(name, dict((k, '%.3g' % v) for k, v in fr.items()))
    for k, v in fr.items():
        # `rule` outputs: at most 1/20 by construction; the double sums and the exact outputs: the float32 evaluation's own figure
        assert v <= (0.05 if S.mode(c, k) == 'rule' else 0.5), (k, v)


# ------------------------------------------------------------------------------------------------ (d) mutants
REJECTED_ON = {
    'pool: row stride 2 Wo on an odd map': ['maxpool/odd_5x7_c4', 'maxpool/odd_5x7_c3', 'maxpool/odd_7x4_c4', 'maxpool/odd_13x13_c32'],
    'pool: tie goes to the last position': ['maxpool/ties_c4', 'maxpool/ties_c3'],
    'lrelu derivative on z': ['bn_bwd_reduce/n64_p64', 'bn_bwd_reduce/n4_p1', 'bn_bwd_apply/hoist_n4'],
    'unbiased variance normalises': ['bn_finalize/n257'],
    'running variance from the biased one': ['bn_finalize/n257', 'bn_finalize/n256_momentum1'],
    'count == 1 divides by zero': ['bn_finalize/n3_count1'],
    'variance not clamped': ['bn_finalize/n3_clamp'],
    'apply: xhat m2 dropped': ['bn_bwd_apply/generic_n12'],
    'apply: m1 and m2 swapped': ['bn_bwd_apply/hoist_n1024'],
    'channel (4 tid) mod N': ['affine_act/vector_affine_n40', 'affine_act/vector_affine_n12', 'affine_act/vector_affine_n2048',
                              'bn_bwd_apply/generic_n12', 'bn_bwd_apply/generic_n2048'],
    'fold: b without running_mean': ['bn_fold/3x3_cin3'],
    'softmax without max subtraction': ['yolo_head/logits_100'],
    'softmax backward without the dot term': ['yolo_head/10_43'],
    'upsample backward sums f terms': ['upsample/f2_c6', 'upsample/f3_c1'],
    'tanh backward on x': ['tanh/range'],
    'permute: scatter equal to gather': ['permute/nchw_to_nhwc_c3', 'permute/nhwc_to_nchw_c32', 'permute/primary_caps_rows'],
    'pick backward writes every class': ['pick/5x43x16', 'pick/d1'],
    'act_bwd: zero takes the positive branch': ['act_bwd/n1000'],
}


def test_every_mutant_has_its_case():
    assert sorted(REJECTED_ON) == sorted(S.MUTANTS)


@pytest.mark.parametrize('mutant,name', [(m, n) for m in sorted(REJECTED_ON) for n in REJECTED_ON[m]])
def test_mutant_is_rejected(mutant, name):
    c = S.case(name)
    got = S.run(c, S.Ref(np.float32, mutant))
    fr = S.fractions(c, got)
    print(mutant, name, dict((k, '%.3g' % v) for k, v in fr.items()))
    assert not S.accepts(c, got), 'the mutant "%s" is not rejected by the case %s' % (mutant, name)
    # and by a wide margin, not at the edge of the tolerance
    assert max(fr.values()) > 5.0, 'the mutant "%s" misses the tolerance of the case %s only narrowly: %s' % (mutant, name, fr)


def test_the_odd_map_defect_in_numbers():
    """What the max-pool of this project computed on a 5 x 7 map before it was handed the cropped tensor: the window addresses of a
    [B][2 Ho][2 Wo][C] tensor on a [B][5][7][C] one."""
    c = S.case('maxpool/odd_5x7_c4')
    bad, ref = S.run(c, S.Ref(np.float64, 'pool: row stride 2 Wo on an odd map')), S.reference(c['name'])
    wrong = int((bad['y'] != ref['y']).sum())
    print('5 x 7 map, 2 images, 4 channels: %d of %d outputs differ' % (wrong, ref['y'].size))
    assert wrong > ref['y'].size // 2


def test_a_mutant_is_a_bug_only_where_it_bites():
    """The switches change nothing where the bug they stand for cannot show: the mutants differ from the reference by their switch alone."""
    for mutant, name in (('pool: row stride 2 Wo on an odd map', 'maxpool/6x10_c4'), ('channel (4 tid) mod N', 'affine_act/hoist_affine_n64_slope0'),
                         ('pool: tie goes to the last position', 'maxpool/6x10_c3'), ('count == 1 divides by zero', 'bn_finalize/n257'),
                         ('softmax without max subtraction', 'yolo_head/logits_80')):
        c = S.case(name)
        assert S.accepts(c, S.run(c, S.Ref(np.float32, mutant))), (mutant, name)

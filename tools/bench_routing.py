"""Times the fused routing kernels (forward and backward, each as launched through the C-ABI) on the heads that matter:
  c1     darkcapsule head      R=g*g*B (5408), N=512,  C=1,  8->5,  cell gather   (BASELINE configs[2])
  caps   CapsuleNet head       R=B (32),       N=1296, C=43, 8->16               (BASELINE configs[0])
  dcn3   DarkCapsuleNet3 head  R=g*g*B (5408), N=512,  C=43, 8->21, cell gather   (stress shape)
  dcn2   DarkCapsuleNet2 head  R=B (32),       N=784,  C=49, 8->48
and heads only the general kernels (csrc/routing_general.hip) take:
  caps100  CapsuleNet, 100 classes            R=B (32),       N=1296, C=100, 8->16
  dcn2g9   DarkCapsuleNet2, 9x9 grid, 10 cl.  R=B (32),       N=784,  C=81,  8->15
  dcn3c80  DarkCapsuleNet3, 80 classes        R=g*g*B (5408), N=512,  C=80,  8->21, cell gather
  din16    16-dim input capsules              R=1024,         N=256,  C=32,  16->32
Prints one JSON object: per shape the mean launch time (HIP events on the launch stream around `reps` back-to-back
calls, plus a cold variant where a 512 MiB buffer is rewritten between calls so that the inputs come from HBM, not from
the Infinity Cache), the algorithmic bytes of SURVEY 8d and the FLOPs the iteration structure needs.

mode: `default` (each shape on the path ops.routing picks), `general` (every shape forced onto the general kernels) or `ab`
(each shape on both paths in the same process, alternating call by call: keys with the suffix _general are the forced-general path).

usage: python3 tools/bench_routing.py [shapes, comma separated | all] [B] [reps] [n_iter] [default | general | ab]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import ops  # noqa: E402

PEAK_HBM = 8000.0      # GB/s
PEAK_F32 = 157.3       # TFLOP/s (vector == fp32 MFMA)


def shapes(B, g=13):
    return {
        'c1': dict(R=g * g * B, N=512, C=1, Din=8, Dout=5, g=g),
        'caps': dict(R=B, N=1296, C=43, Din=8, Dout=16, g=0),
        'dcn3': dict(R=g * g * B, N=512, C=43, Din=8, Dout=21, g=g),
        'dcn2': dict(R=B, N=784, C=49, Din=8, Dout=48, g=0),
        'caps100': dict(R=B, N=1296, C=100, Din=8, Dout=16, g=0),
        'dcn2g9': dict(R=B, N=784, C=81, Din=8, Dout=15, g=0),
        'dcn3c80': dict(R=g * g * B, N=512, C=80, Din=8, Dout=21, g=g),
        'din16': dict(R=1024, N=256, C=32, Din=16, Dout=32, g=0),
    }


def algorithmic(s, r):
    R, N, C, Din, Dout = s['R'], s['N'], s['C'], s['Din'], s['Dout']
    fwd_b = 4.0 * (R * N * Din + N * C * Din * Dout + R * C * Dout)
    bwd_b = 4.0 * (2 * R * N * Din + 2 * N * C * Din * Dout + R * C * Dout)
    trip = float(R) * N * C
    # u_hat is recomputed in every iteration (it cannot be kept: R*N*C*Dout floats); per (row, i, j) and iteration:
    # prediction 2*Din*Dout, logit 2*Dout, weighted sum 2*Dout (+ ~8 for the softmax)
    fwd_f = trip * (r * 2 * Din * Dout + (r - 1) * 2 * Dout + r * 2 * Dout + 8 * (r - 1)) if C > 1 else trip * 2 * Din * Dout
    return fwd_b, bwd_b, fwd_f


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else 'all'
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    r = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    mode = sys.argv[5] if len(sys.argv) > 5 else 'default'
    assert mode in ('default', 'general', 'ab'), mode
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    sh = shapes(B)
    names = list(sh) if which == 'all' else which.split(',')
    trash = torch.empty(128 * 1024 * 1024, device=dev)     # 512 MiB: evicts the 256 MiB Infinity Cache
    out = {'B': B, 'n_iter': r, 'reps': reps, 'mode': mode, 'shapes': {}}
    for name in names:
        s = sh[name]
        g = s['g']
        if g:
            u = torch.randn(B, 4 * g, 4 * g, 256, device=dev)
        else:
            u = torch.randn(s['R'], s['N'], s['Din'], device=dev)
        W = 0.1 * torch.randn(1, s['N'], s['C'], s['Din'], s['Dout'], device=dev)
        res = {'shape': s}
        try:
            u.requires_grad_(True)
            W.requires_grad_(True)
            for gen in ([False, True] if mode == 'ab' else [mode == 'general']):     # warm-up of every path timed below
                ops.ROUTING_FORCE_GENERAL = gen
                v = ops.routing(u, W, r, g, B if g else 0)
                gv = torch.randn_like(v)
                torch.autograd.grad(v, (u, W), gv)
            ops.ROUTING_FORCE_GENERAL = False
            torch.cuda.synchronize()

            def timed(fn, cold, general=None):
                ts = {}
                paths = [False, True] if general is None else [general]
                for _ in range(reps):
                    for gen in paths:             # both paths: alternating call by call
                        ops.ROUTING_FORCE_GENERAL = gen
                        if cold:
                            trash.fill_(1.0)
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn()
                        b.record()
                        torch.cuda.synchronize()
                        ts.setdefault(gen, []).append(a.elapsed_time(b))
                ops.ROUTING_FORCE_GENERAL = False
                return dict((k, sorted(v)[len(v) // 2]) for k, v in ts.items())

            ud, Wd = u.detach(), W.detach()
            ops.timer.enabled = False
            fixed = None if mode == 'ab' else (mode == 'general')

            def fb():
                vv = ops.routing(u, W, r, g, B if g else 0)
                torch.autograd.grad(vv, (u, W), gv)
            f_warm = timed(lambda: ops.routing(ud, Wd, r, g, B if g else 0), False, fixed)
            f_cold = timed(lambda: ops.routing(ud, Wd, r, g, B if g else 0), True, fixed)
            fb_warm = timed(fb, False, fixed)
            fb_cold = timed(fb, True, fixed)
            fwd_b, bwd_b, fwd_f = algorithmic(s, r)
            res.update({'fwd_bytes': int(fwd_b), 'bwd_bytes': int(bwd_b), 'fwd_flops': fwd_f})
            for gen in f_warm:
                sfx = '_general' if (gen and mode == 'ab') else ''
                res.update({'fwd_ms_warm' + sfx: round(f_warm[gen], 5), 'fwd_ms_cold' + sfx: round(f_cold[gen], 5),
                            'fwd_bwd_ms_warm' + sfx: round(fb_warm[gen], 5), 'fwd_bwd_ms_cold' + sfx: round(fb_cold[gen], 5),
                            'bwd_ms_warm' + sfx: round(fb_warm[gen] - f_warm[gen], 5),
                            'fwd_hbm_frac_cold' + sfx: round(fwd_b / (f_cold[gen] * 1e-3) / 1e9 / PEAK_HBM, 4),
                            'fwd_hbm_frac_warm' + sfx: round(fwd_b / (f_warm[gen] * 1e-3) / 1e9 / PEAK_HBM, 4),
                            'fwd_f32_frac_cold' + sfx: round(fwd_f / (f_cold[gen] * 1e-3) / 1e12 / PEAK_F32, 4),
                            'fwd_f32_frac_warm' + sfx: round(fwd_f / (f_warm[gen] * 1e-3) / 1e12 / PEAK_F32, 4)})
        except Exception as e:                 # an unsupported shape is reported, not hidden
            res['error'] = str(e)[:300]
        out['shapes'][name] = res
        del u, W
    print(json.dumps(out))


if __name__ == '__main__':
    main()

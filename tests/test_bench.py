"""bench.py's own contract: --steps sets the timed steps, a plain run prints only the headline, --dump-outputs writes what
the last timed step computed, and the same arguments give the same inputs from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import REPO


def _bench(args, timeout=600):
    env = dict(os.environ, PYTHONUNBUFFERED='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(REPO, 'bench.py')] + args, env=env, cwd=REPO, capture_output=True,
                          text=True, timeout=timeout)


def test_bench_rejects_zero_timed_steps():
    r = _bench(['--steps', '0'], timeout=120)
    assert r.returncode == 2 and '--steps must be >= 1' in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    d = tmp_path / 'out'
    r = _bench(['--gpus', '1', '--batch', '2', '--input', '64', '--steps', '3', '--warmup', '1', '--dump-outputs', str(d)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'images/s' and line['dtype'] == 'f32'
    assert line['higher_is_better'] is True and line['metric']
    assert np.isfinite(line['ms_per_step']) and line['ms_per_step'] > 0
    assert abs(line['value'] - 2 * 1e3 / line['ms_per_step']) <= 1e-3 * line['value']
    for k in ('roofline', 'roofline_routing', 'pcie_inclusive', 'kernel_ms', 'roofline_routing_c43', 'loss_curve_parity',
              'secondary', 'cpu_baseline'):
        assert k not in line, k                                   # --full only
    files = sorted(os.listdir(d))
    arrays = dict((f[:-4], np.load(os.path.join(d, f))) for f in files)
    assert all(f.endswith('.npy') for f in files) and sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays['output'].shape == (2, 2, 2, 5)
    assert arrays['loss'].shape == (1,) and abs(float(arrays['loss'][0]) - line['config']['final_loss']) <= 1e-6
    assert arrays['param.traffic_sign_capsules.route_weights'].shape == (1, 512, 1, 8, 5)
    assert arrays['grad.conv.conv_2.weight'].shape == arrays['param.conv.conv_2.weight'].shape == (256, 128, 3, 3)
    assert arrays['buffer.conv.bn_5.running_var'].shape == (256,)

    # the same four steps split 3 + 1 instead of 1 + 3: identical inputs and initialisation from run to run, so the last step
    # computes the same loss, output and parameters -- and only --steps / --warmup decide how many steps run (1 + 1 differs)
    d2 = tmp_path / 'out2'
    r = _bench(['--gpus', '1', '--batch', '2', '--input', '64', '--steps', '1', '--warmup', '3', '--dump-outputs', str(d2)])
    assert r.returncode == 0, r.stderr[-3000:]
    line2 = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    loss4 = line['config']['final_loss']
    assert line2['steps'] == 1 and line2['warmup'] == 3 and abs(line2['config']['final_loss'] - loss4) <= 1e-5 * abs(loss4)
    assert sorted(os.listdir(d2)) == files
    for name, a in arrays.items():
        b = np.load(os.path.join(d2, name + '.npy'))
        np.testing.assert_allclose(b, a, rtol=1e-5, atol=1e-6 * max(1e-30, float(np.abs(a).max())), err_msg=name)
    r = _bench(['--gpus', '1', '--batch', '2', '--input', '64', '--steps', '1', '--warmup', '1'])
    assert r.returncode == 0, r.stderr[-3000:]
    line3 = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert line3['steps'] == 1 and abs(line3['config']['final_loss'] - loss4) > 1e-3 * abs(loss4)

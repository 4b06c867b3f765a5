"""CPU-side tests of the shared launch arithmetic (csrc/common.h) and device primitives (csrc/prims.h): what the workspace queries
answer when no device can be asked for its CU count, the gate in front of the wrong-result developer knobs, one copy of every primitive."""
import os
import re
import subprocess
import sys

import pytest

from helpers import REPO

PKG = os.path.join(REPO, 'cs231-capsule-yolo-traffic-sign-detection_amd')
CSRC = os.path.join(PKG, 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'

# (entry point, arguments, value without a device).  The three policies of a failed CU-count query: cy_wino4_wgrad_ws_floats assumes 256
# CUs (ncu / per blocks per tile range, capped by the chunk pairs: the first and the third shape hit the cap, the second ncu / per);
# cy_wino_split_ws_floats does not split; the other two never ask.
NO_DEVICE = [
    ('cy_wino4_wgrad_ws_floats', (2, 16, 32, 32, 64), 589824),
    ('cy_wino4_wgrad_ws_floats', (32, 208, 208, 128, 128), 18874368),
    ('cy_wino4_wgrad_ws_floats', (1, 4, 16, 32, 64), 73728),
    ('cy_wino_split_ws_floats', (16, 13, 13, 1024, 512, 1), 0),
    ('cy_wino_split_ws_floats', (16, 13, 13, 1024, 512, 0), 0),
    ('cy_wino_wgrad_ws_floats', (16, 64, 64), 16778240),
    ('cy_wino_wgrad_ws_floats', (32, 128, 128), 16778240),
    ('cy_wino2_wgrad_ws_floats', (4, 128, 256), 18874368),
]

_CHILD = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
out = []
for name, args in json.loads(sys.argv[2]):
    f = getattr(lib, name)
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_int] * len(args)
    out.append(f(*args))
print(json.dumps(out))
'''


def test_workspace_queries_without_a_device():
    """The workspace-size queries are host arithmetic and run where no device answers (a child process that sees none, so that the
    test asks the same question on a GPU machine): each keeps its policy for a CU count that cannot be had."""
    import json
    from capsyolo_amd import _lib
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    r = subprocess.run([sys.executable, '-c', _CHILD, _lib.LIB_PATH, json.dumps([(n, a) for n, a, _ in NO_DEVICE])],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == [v for _, _, v in NO_DEVICE], list(zip(NO_DEVICE, got))


# every developer knob whose nonzero value compiles kernels with wrong results, and the unit that defines it
GATED_KNOBS = [('CY_F4_DBG', 'winograd4.hip'), ('CY_G4_DBG', 'winograd4_wgrad.hip'), ('CY_WINO_DBG', 'winograd.hip'),
               ('W2_SKIP', 'winograd_s2.hip'), ('CY_WG_DBG', 'conv_bf16.hip'), ('CY_BF_DBG', 'conv_bf16.hip'),
               ('CY_BF_NOSTAGGER', 'conv_bf16.hip'), ('CY_ROWS_DBG', 'routing_rows.hip'), ('CY_B2_DBG', 'routing_caps.hip')]


@pytest.mark.parametrize('knob,unit', GATED_KNOBS)
def test_wrong_result_knobs_need_a_dev_build(knob, unit):
    """A plain -D<knob>=1 does not compile: the error names the knob and the way out.  With -DCY_DEV_BUILD the same line compiles."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    line = [HIPCC, '-std=c++17', '--offload-arch=gfx950', '-I' + os.path.join(REPO, 'include'), '-fsyntax-only', '--cuda-device-only',
            '-Wfatal-errors', '-D%s=1' % knob, os.path.join(CSRC, unit)]
    r = subprocess.run(line, capture_output=True, text=True)
    assert r.returncode != 0
    assert re.search(r'error: static assertion failed.*\b%s\b.*CY_DEV_BUILD' % knob, r.stderr), r.stderr[-2000:]
    r = subprocess.run(line[:-1] + ['-DCY_DEV_BUILD', line[-1]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_every_gated_knob_is_listed():
    """The units' comments mark these knobs with `results are wrong`: each such unit invokes the gate for each knob it defines."""
    for unit in sorted(u for u in os.listdir(CSRC) if u.endswith(('.hip', '.h'))):
        src = open(os.path.join(CSRC, unit)).read()
        gated = set(re.findall(r'^CY_WRONG_RESULT_KNOB\((\w+)\);', src, re.M))
        assert gated == {k for k, u in GATED_KNOBS if u == unit}, unit
        if unit.endswith('.hip'):
            assert bool(gated) == bool(re.search(r'results are wrong', src)), unit


def test_device_primitives_exist_once():
    """No private copy of a primitive of prims.h in a unit: none of the retired names, one wrapper per instruction."""
    retired = re.compile(r'\b(i32x4_|i32x4h_|i32x4g_|wg_i32x4|h4_mfma|g4_mfma_a|wg_store)\b')
    once = ['v_accvgpr_read_b32', 'buffer_store_dwordx4', 'buffer_load_dwordx4 %0', 'global_load_dwordx4 %0, %1, %2 offset', 'v_mfma_f32_16x16x4_f32',
            'ds_read2st64_b32', 's_waitcnt vmcnt(%1)']
    for unit in sorted(os.listdir(CSRC)):
        if unit == 'prims.h' or not unit.endswith(('.hip', '.h')):
            continue
        code = re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, unit)).read())
        assert not retired.search(code), (unit, retired.search(code).group(0))
        for ins in once:
            assert ins not in code, (unit, ins)
    prims = re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, 'prims.h')).read())
    assert prims.count('v_accvgpr_read_b32') == 1 and prims.count('buffer_store_dwordx4') == 1 and prims.count('s_nop 1') == 1

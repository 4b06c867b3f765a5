"""The routing plan (csrc/routing.hip cyi_routing_plan, exported as cy_routing_plan / ops.routing_plan): which path takes a call,
with which launch numbers, and how the workspace is carved into regions.  The launchers take every pointer from these regions and
the _ws_floats queries return the plan's total, so a region that overlaps another or ends past the total is a kernel writing outside
its workspace.  Host arithmetic: no GPU.  The built and the new heads are pinned literally: the values the library had before the
plan existed (totals from its workspace queries, the other fields from a build of it with a print added); the phased backward totals
are those minus the R * C * Dout plane that nothing read."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from helpers import REPO
from test_routing_general_host import BUILT_HEADS, ENVELOPE, NEW_HEADS, ORACLE_SHAPES, OUTSIDE, bwd, fwd, q

from capsyolo_amd import _lib, ops

ALL = BUILT_HEADS + NEW_HEADS + [s + (0, 0) for s in ORACLE_SHAPES + ENVELOPE]


def plan(shape, backward=False, force=False):
    return ops.routing_plan(*shape, backward=backward, force_general=force)


def fields(p):
    return (p['path'], p['row_blocks'], p['nch'], p['ic'], p['cdb'], p['total'])


@pytest.mark.parametrize('shape', ALL)
def test_regions_tile_the_workspace_of_the_matching_query(shape):
    R, N, Cc, Din, Dout, n_iter = shape[:6]
    specialised = q('cy_routing_specialised', fwd(*shape))
    for backward in (False, True):
        for force in (False, True):
            p = plan(shape, backward, force)
            general = p['path'] == 'general'
            assert general == bool(force or not specialised), (shape, backward, force, p)
            end = 0
            for name, off, n in p['regions']:                      # ordered, no overlap, nothing empty
                assert off >= end and n > 0, (shape, backward, force, p)
                end = off + n
            assert p['total'] == end
            names = [r[0] for r in p['regions']]
            assert len(set(names)) == len(names)
            where = {name: off for name, off, n in p['regions']}
            # 16-byte boundaries: the packed W image everywhere, V and the slabs of a forward, every region of the general kernels
            for name, off in where.items():
                if name == 'W' or not backward or general:
                    assert off % 4 == 0, (shape, backward, force, name, p)
            a = bwd(*shape) if backward else fwd(*shape)
            d = 'bwd' if backward else 'fwd'
            if general:
                assert p['total'] == q('cy_routing_general_%s_ws_floats' % d, a)
            if not force:
                assert p['total'] == q('cy_routing_%s_ws_floats' % d, a)
            if backward and not general and p['path'] != 'c1':     # csrc/routing_caps.hip reads these two without the plan
                assert p['regions'][0] == ('ds_all', 0, n_iter * R * Cc * Dout)
                assert p['regions'][1] == ('V_all', n_iter * R * Cc * Dout, n_iter * R * Cc * Dout)
                assert 'tail' in where and where['tail'] >= 2 * n_iter * R * Cc * Dout
            assert p['cdb'] == ('cdb' in where)


# shape -> (path, row blocks, chunks of input capsules, capsules per chunk, cdb saved, total) of the forward and of the backward
PINNED = {
    (5408, 512, 1, 8, 5, 3, 13, 32): (('c1', 256, 1, 512, False, 0), ('c1', 256, 1, 512, False, 5242880)),
    (32, 1296, 43, 8, 16, 3, 0, 0): (('rows_phased', 1, 216, 6, False, 12740096), ('rows_phased', 1, 216, 6, False, 12287684 - 22016)),
    (5408, 512, 43, 8, 21, 3, 13, 32): (('rows_fused', 226, 1, 512, False, 4718592), ('rows_fused', 338, 1, 512, True, 509513540)),
    (32, 784, 49, 8, 48, 3, 0, 0): (('rows_phased', 4, 61, 13, False, 19571776), ('rows_phased', 4, 61, 13, False, 20098628 - 75264)),
    (32, 1296, 100, 8, 16, 3, 0, 0): (('general', 16, 62, 21, False, 24459264), ('general', 16, 62, 21, False, 91121664)),
    (32, 784, 81, 8, 15, 3, 0, 0): (('general', 16, 61, 13, False, 15416320), ('general', 16, 61, 13, False, 48179200)),
    (5408, 512, 80, 8, 21, 3, 13, 32): (('general', 2704, 1, 512, False, 33349632), ('general', 2704, 1, 512, False, 162143232)),
    (1024, 256, 32, 16, 32, 3, 0, 0): (('general', 256, 4, 64, False, 13631488), ('general', 256, 4, 64, False, 95420416)),
}
# the built heads on the general kernels (the new heads are there anyway)
PINNED_FORCED = {
    (5408, 512, 1, 8, 5, 3, 13, 32): (('general', 1352, 1, 512, False, 2183680), ('general', 1352, 1, 512, False, 28710912)),
    (32, 1296, 43, 8, 16, 3, 0, 0): (('general', 8, 118, 11, False, 13236736), ('general', 8, 118, 11, False, 41901568)),
    (5408, 512, 43, 8, 21, 3, 13, 32): (('general', 1352, 1, 512, False, 17453568), ('general', 1352, 1, 512, False, 122073600)),
    (32, 784, 49, 8, 48, 3, 0, 0): (('general', 8, 112, 7, False, 27772416), ('general', 8, 112, 7, False, 87230976)),
}


@pytest.mark.parametrize('shape', BUILT_HEADS + NEW_HEADS)
def test_heads_keep_their_plan(shape):
    assert set(PINNED) == set(BUILT_HEADS + NEW_HEADS) and set(PINNED_FORCED) == set(BUILT_HEADS)
    assert (fields(plan(shape)), fields(plan(shape, backward=True))) == PINNED[shape]
    forced = PINNED_FORCED.get(shape, PINNED[shape])
    assert (fields(plan(shape, force=True)), fields(plan(shape, backward=True, force=True))) == forced


def test_plan_boundaries():
    # many rows: one fused launch; few rows: a pass and a finish per iteration over chunks of input capsules
    assert fields(plan((1100, 12, 5, 8, 16, 3))) == ('rows_fused', 138, 1, 12, False, 24576)
    assert fields(plan((1100, 12, 5, 8, 16, 3), backward=True)) == ('rows_fused', 138, 1, 12, True, 799924)
    assert fields(plan((37, 70, 43, 8, 16, 3))) == ('rows_phased', 2, 35, 2, False, 1346496)
    assert fields(plan((37, 70, 43, 8, 16, 3), backward=True)) == ('rows_phased', 2, 35, 2, False, 1491932 - 25456)
    # the fused backward saves the couplings for the du / dW kernel up to Dout 21, not at 48
    assert fields(plan((1100, 20, 43, 8, 21, 4), backward=True)) == ('rows_fused', 138, 1, 20, True, 13777204)
    assert fields(plan((1040, 10, 49, 8, 48, 2), backward=True)) == ('rows_fused', 208, 1, 10, False, 9974444)
    assert fields(plan((1100, 20, 43, 8, 21, 1), backward=True))[4] is False                  # one iteration: nothing to save
    # C = 64 is the last specialised capsule count
    assert fields(plan((5, 64, 64, 8, 16, 3))) == ('rows_phased', 1, 32, 2, False, 709632)
    assert fields(plan((5, 64, 65, 8, 16, 3))) == ('general', 3, 16, 4, False, 1136976)
    assert fields(plan((5, 64, 64, 8, 16, 3), backward=True)) == ('rows_phased', 1, 32, 2, False, 745476 - 5120)
    assert fields(plan((5, 64, 65, 8, 16, 3), backward=True)) == ('general', 3, 16, 4, False, 1500976)


def test_mfma_forward_is_chosen_by_the_environment_in_the_plan():
    """CY_ROUTING_MFMA=1 (read by the plan and nowhere else) moves the forward of the shapes routing_mfma.hip takes, and only those;
    the workspace is the same either way (the larger of the two W images is always reserved)."""
    code = ('import sys; sys.path.insert(0, %r); from capsyolo_amd import ops\n'
            'for s in [(32, 1296, 43, 8, 16, 3), (32, 1296, 43, 8, 5, 3), (1100, 12, 5, 8, 16, 3)]:\n'
            '    p = ops.routing_plan(*s); b = ops.routing_plan(*s, backward=True)\n'
            '    print(p["path"], p["row_blocks"], p["nch"], p["ic"], p["total"], b["path"])\n' % REPO)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, CY_ROUTING_MFMA='1'), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split('\n')[:3] == ['mfma_phased 2 118 11 12740096 rows_phased', 'rows_phased 1 216 6 4390816 rows_phased',
                                        'mfma_fused 69 1 12 24576 rows_fused']
    if os.environ.get('CY_ROUTING_MFMA', '') != '1':
        assert plan((32, 1296, 43, 8, 16, 3))['path'] == 'rows_phased'


@pytest.mark.parametrize('shape', OUTSIDE + [(8, 512, 80, 4, 21, 3, 2, 2), (9, 512, 80, 8, 21, 3, 2, 2)])
def test_no_plan_outside_the_envelope(shape):
    out = (C.c_longlong * 34)()
    for backward in (0, 1):
        for force in (0, 1):
            assert _lib.query('cy_routing_plan', C.byref(fwd(*shape)), backward, force, out, 34) != 0
            assert b'cy_routing_plan' in _lib.query('capsyolo_last_error')
    assert q('cy_routing_fwd_ws_floats', fwd(*shape)) == 0 and q('cy_routing_bwd_ws_floats', bwd(*shape)) == 0


def test_envelope_message_comes_from_the_plan():
    with pytest.raises(_lib.HipExtensionError, match='envelope') as e:
        plan((4, 10, 300, 8, 16, 3))
    assert 'Din 1..16' in str(e.value) and 'Dout 1..64' in str(e.value) and 'C 1..256' in str(e.value)
    out = (C.c_longlong * 7)()
    assert _lib.query('cy_routing_plan', C.byref(fwd(37, 70, 43, 8, 16, 3)), 1, 0, out, 7) != 0     # too short for the region table

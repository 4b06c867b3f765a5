"""Host logic of the general routing kernels (csrc/routing_general.hip): which shapes the specialised kernels keep, and the
workspace queries of the general entry points inside and outside their envelope.  No GPU needed."""
import ctypes as C

import pytest

from capsyolo_amd import _lib

# the four heads of tools/bench_routing.py (B = 32, g = 13)
BUILT_HEADS = [(5408, 512, 1, 8, 5, 3, 13, 32), (32, 1296, 43, 8, 16, 3, 0, 0), (5408, 512, 43, 8, 21, 3, 13, 32),
               (32, 784, 49, 8, 48, 3, 0, 0)]
# every shape of tests/test_gpu_kernels.py::test_routing_vs_oracle
ORACLE_SHAPES = [(37, 70, 43, 8, 16, 3), (9, 33, 7, 8, 21, 2), (130, 512, 1, 8, 5, 3), (5, 64, 64, 8, 16, 3), (3, 20, 3, 8, 5, 4),
                 (1100, 12, 5, 8, 16, 3), (600, 10, 7, 8, 21, 2), (1030, 9, 3, 8, 5, 3), (1100, 20, 43, 8, 21, 4),
                 (1100, 16, 20, 8, 16, 5), (1050, 8, 6, 8, 21, 6), (1040, 10, 49, 8, 48, 2), (32, 1296, 43, 8, 16, 3),
                 (6, 40, 49, 8, 48, 3), (5, 30, 4, 8, 48, 2), (4, 24, 20, 8, 48, 3), (70, 300, 43, 8, 21, 3), (200, 64, 33, 8, 16, 3)]
# the new heads of tools/bench_routing.py: caps100, dcn2g9, dcn3c80, din16
NEW_HEADS = [(32, 1296, 100, 8, 16, 3, 0, 0), (32, 784, 81, 8, 15, 3, 0, 0), (5408, 512, 80, 8, 21, 3, 13, 32),
             (1024, 256, 32, 16, 32, 3, 0, 0)]
# shapes of the envelope's corners (R, N, C, Din, Dout, n_iter)
ENVELOPE = [(1, 1, 1, 1, 1, 1), (2, 37, 256, 16, 64, 7), (1000, 1, 65, 16, 15, 3), (3, 1296, 2, 4, 3, 2), (1, 5, 256, 1, 1, 1)]
OUTSIDE = [(4, 10, 257, 8, 16, 3), (4, 10, 43, 17, 16, 3), (4, 10, 43, 8, 65, 3), (4, 10, 43, 0, 16, 3), (0, 10, 43, 8, 16, 3),
           (4, 10, 43, 8, 16, 0)]


def fwd(R, N, Cc, Din, Dout, n_iter, g=0, B=0):
    return _lib.RoutingFwd(R=R, N=N, C=Cc, Din=Din, Dout=Dout, n_iter=n_iter, gather_g=g, gather_B=B)


def bwd(R, N, Cc, Din, Dout, n_iter, g=0, B=0):
    return _lib.RoutingBwd(R=R, N=N, C=Cc, Din=Din, Dout=Dout, n_iter=n_iter, gather_g=g, gather_B=B)


def q(name, a):
    return _lib.query(name, C.byref(a))


@pytest.mark.parametrize('shape', BUILT_HEADS + [s + (0, 0) for s in ORACLE_SHAPES])
def test_built_shapes_stay_specialised(shape):
    assert q('cy_routing_specialised', fwd(*shape)) == 1


@pytest.mark.parametrize('shape', NEW_HEADS + [s + (0, 0) for s in ENVELOPE if s[2] > 64 or s[3] != 8])
def test_other_shapes_are_not_specialised(shape):
    assert q('cy_routing_specialised', fwd(*shape)) == 0


@pytest.mark.parametrize('shape', NEW_HEADS + BUILT_HEADS + [s + (0, 0) for s in ENVELOPE])
def test_general_workspace_inside_the_envelope(shape):
    R, N, Cc, Din, Dout, n_iter = shape[:6]
    nf, nb = q('cy_routing_general_fwd_ws_floats', fwd(*shape)), q('cy_routing_general_bwd_ws_floats', bwd(*shape))
    # at least the packed W image and, backward, V_t and ds^t of every iteration
    assert nf >= N * Din * Dout * Cc + R * Cc * Dout
    assert nb >= N * Din * Dout * Cc + 2 * n_iter * R * Cc * Dout
    if not q('cy_routing_specialised', fwd(*shape)):      # the classic queries hand out the general workspace for these
        assert q('cy_routing_fwd_ws_floats', fwd(*shape)) == nf
        assert q('cy_routing_bwd_ws_floats', bwd(*shape)) == nb


@pytest.mark.parametrize('shape', OUTSIDE + [(8, 512, 80, 4, 21, 3, 2, 2), (9, 512, 80, 8, 21, 3, 2, 2)])
def test_general_workspace_outside_the_envelope(shape):
    assert q('cy_routing_general_fwd_ws_floats', fwd(*shape)) < 0
    msg = _lib.load().capsyolo_last_error().decode()
    assert 'cy_routing_general_fwd_ws_floats' in msg
    assert q('cy_routing_general_bwd_ws_floats', bwd(*shape)) < 0
    assert q('cy_routing_specialised', fwd(*shape)) == 0


def test_envelope_message_names_the_envelope():
    assert q('cy_routing_general_fwd_ws_floats', fwd(4, 10, 300, 8, 16, 3)) < 0
    msg = _lib.load().capsyolo_last_error().decode()
    assert 'Din 1..16' in msg and 'Dout 1..64' in msg and 'C 1..256' in msg, msg


def test_new_entry_points_are_bound():
    for n in ('cy_routing_general_fwd', 'cy_routing_general_bwd', 'cy_routing_general_fwd_ws_floats',
              'cy_routing_general_bwd_ws_floats', 'cy_routing_specialised', 'cy_routing_plan'):
        assert n in _lib.EXPORTS and hasattr(_lib.load(), n)

"""CPU-side tests of cy_adam_step (csrc/adam.hip), the one entry point of optim.Adam's step: its declaration, that the eight entry points
it replaced are gone from header, bindings and library, its argument checks (every refusal comes before a launch, so none needs a
GPU), and the trace label of _lib.call."""
import ctypes as C
import os
import re

import pytest

from helpers import REPO

import capsyolo_amd  # noqa: F401
from capsyolo_amd import _lib

OLD = ['cy_adam_multi' + dev + clip + ema for dev in ('', '_dev') for clip in ('', '_clip') for ema in ('', '_ema')]


def test_one_entry_point_and_none_of_the_eight():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    decl = re.search(r'\bint cy_adam_step\(([^;]*)\);', header, re.S)
    assert decl, 'cy_adam_step is not declared in capsyolo_hip.h'
    assert len(re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')) == 2
    assert 'cy_adam_step' in _lib.EXPORTS and hasattr(lib, 'cy_adam_step')
    assert len(_lib._SIGS['cy_adam_step']) == 2
    assert len(OLD) == 8 and len(set(OLD)) == 8
    assert 'cy_adam_multi' not in header
    for name in OLD:
        assert name not in _lib.EXPORTS and name not in _lib._SIGS, name
        assert not hasattr(lib, name), '%s is still a symbol of the library' % name
    assert lib.capsyolo_abi_version() == _lib.ABI_VERSION == 6


def _step(**kw):
    """A descriptor that passes every check (host scalars, no record, no average) with the fields of kw changed.  The pointers are never
    followed: every call here is refused before the launch."""
    a = dict(table=64, blockmap=64, n_blocks=1, chunk=16384, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bias_corr1=0.1, bias_corr2=0.001,
             one_minus_decay=0.0)
    a.update(kw)
    return _lib.AdamStep(**a)


@pytest.mark.parametrize('field,kw', [
    ('table', dict(table=None)),
    ('blockmap', dict(blockmap=None)),
    ('n_blocks', dict(n_blocks=0)),
    ('chunk', dict(chunk=0)),
    ('bias_corr1', dict(bias_corr1=0.0)),
    ('bias_corr2', dict(bias_corr2=0.0)),
    ('one_minus_decay', dict(ema_table=64, one_minus_decay=0.0)),
    ('one_minus_decay', dict(ema_table=64, one_minus_decay=1.5)),
    ('one_minus_decay', dict(ema_table=64, one_minus_decay=float('nan'))),
], ids=['table', 'blockmap', 'n_blocks', 'chunk', 'bias_corr1', 'bias_corr2', 'decay_0', 'decay_1.5', 'decay_nan'])
def test_refusals_name_the_field(field, kw):
    lib = _lib.load()
    a = _step(**kw)
    assert lib.cy_adam_step(C.byref(a), None) != 0
    msg = lib.capsyolo_last_error().decode()
    assert msg.startswith('cy_adam_step:') and field in msg, msg
    others = set(['table', 'blockmap', 'n_blocks', 'chunk', 'bias_corr1', 'bias_corr2', 'one_minus_decay']) - set([field])
    assert not any(re.search(r'\b%s\b' % o, msg) for o in others), msg
    with pytest.raises(_lib.HipExtensionError, match=r'cy_adam_step failed \(code \d+\): cy_adam_step: .*%s' % field):
        _lib.call('cy_adam_step', C.byref(a), None)


def test_call_appends_the_label_or_the_name():
    a = _step(n_blocks=0)
    _lib.TRACE = trace = []
    try:
        for kw in (dict(trace='x'), dict(), dict(trace='cy_adam_step+dev+ema'), dict(trace=None)):
            with pytest.raises(_lib.HipExtensionError):
                _lib.call('cy_adam_step', C.byref(a), None, **kw)
    finally:
        _lib.TRACE = None
    assert trace == ['x', 'cy_adam_step', 'cy_adam_step+dev+ema', 'cy_adam_step']
    with pytest.raises(_lib.HipExtensionError):                          # and nothing with the census off
        _lib.call('cy_adam_step', C.byref(a), None, trace='x')
    assert trace == ['x', 'cy_adam_step', 'cy_adam_step+dev+ema', 'cy_adam_step'] and _lib.TRACE is None

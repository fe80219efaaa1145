"""The entry points of the streamed-weights beam search (include/arvae_hip.h, arvae_tick_beam_search_wide*) without a GPU: the
symbols, what the predicates answer, and that every argument check refuses with its message before anything is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('arvae_tick_beam_search_wide_supported', 'arvae_tick_beam_search_wide_ws_floats', 'arvae_tick_beam_search_wide',
         'arvae_tick_beam_search_wide_planned', 'arvae_tick_beam_search_wide_groups')


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_symbols_are_bound_and_declared_once(lib):
    from arvae_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'arvae_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(re.findall(r'^int(?:64_t)? ' + name + r'\(', header, re.M)) == 1, name
    assert lib.arvae_abi_version() == 16 == _lib.ABI_VERSION     # symbols added, nothing existing changed: the number stays
    assert re.search(r'#define ARVAE_ABI_VERSION\s+16\b', header)


def test_predicates(lib):
    from arvae_amd import ops
    sup = lib.arvae_tick_beam_search_wide_supported
    for hid in (256, 512):
        for vocab in (2, 35, 128):
            for width in range(1, 17):
                for groups in range(0, 18):
                    want = groups <= width and (groups == 0 or width % groups == 0)
                    assert sup(hid, vocab, width, groups) == int(want), (hid, vocab, width, groups)
        # just outside each bound
        assert sup(hid, 1, 4, 1) == 0 and sup(hid, 129, 4, 1) == 0
        assert sup(hid, 35, 0, 0) == 0 and sup(hid, 35, 17, 1) == 0 and sup(hid, 35, -1, 1) == 0
        assert sup(hid, 35, 4, 3) == 0 and sup(hid, 35, 4, 5) == 0 and sup(hid, 35, 4, -1) == 0
    for hid in (128, 255, 257, 384, 511, 513, 1024):
        assert sup(hid, 35, 4, 1) == 0
    assert ops.tick_beam_search_wide_supported(512, 35, 4) and ops.tick_beam_search_wide_supported(256, 35, 8, 4)
    assert not ops.tick_beam_search_wide_supported(128, 35, 4) and not ops.tick_beam_search_wide_supported(512, 35, 8, 3)
    # the one-launch searches answer what they answered
    assert lib.arvae_tick_beam_search_supported(128, 35, 4) == 1 and lib.arvae_tick_beam_search_supported(256, 35, 4) == 0
    assert lib.arvae_tick_beam_search_groups_supported(512, 35, 8, 4) == 0


def test_workspace_size(lib):
    ws = lib.arvae_tick_beam_search_wide_ws_floats                          # (batch, ticks, hidden, vocab, width)
    assert ws(0, 24, 256, 35, 4) == -1 and ws(5, 0, 256, 35, 4) == -1 and ws(5, 24, 128, 35, 4) == -1 and ws(5, 24, 384, 35, 4) == -1
    assert ws(5, 24, 256, 1, 4) == -1 and ws(5, 24, 256, 129, 4) == -1 and ws(5, 24, 256, 35, 0) == -1 and ws(5, 24, 256, 35, 17) == -1
    assert ws(1 << 28, 24, 256, 35, 16) == -1                  # more rows than an int32 counts
    sizes = [ws(b, 24, 256, 35, 4) for b in (1, 5, 37, 256, 257)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(5, 24, 512, 35, 4) > ws(5, 24, 256, 35, 4) and ws(5, 24, 256, 35, 8) > ws(5, 24, 256, 35, 4)
    assert ws(5, 48, 256, 35, 4) > ws(5, 24, 256, 35, 4) and ws(5, 24, 256, 70, 4) > ws(5, 24, 256, 35, 4)
    rows, ticks = 5 * 4, 24                                     # the states of two ticks, a tick's logits, the history
    assert ws(5, 24, 256, 35, 4) >= 4 * rows * 256 + rows * 35 + 3 * rows + 4 * ticks * rows
    assert ws(1 << 22, 24, 512, 35, 16) > 4 * (1 << 26) * 512   # 64-bit


def _calls(lib, base):
    """the three entry points as functions of keyword overrides of one complete, acceptable argument list whose pointers are host
    addresses that are never dereferenced"""
    from arvae_amd import _lib
    good = ctypes.c_void_p(base)
    common = dict(weights=_lib.TickWeights(*[base] * 8), h0_l0=good, h0_l1=good, h0_stride=0, gib=good, ptab=good, batch=5, beats=4, tpb=6,
                  hidden=256, vocab=35, width=4, allow=None, allowed=35, plan=_lib.NotePlan(base, 24 * 35, 35), groups=2, penalty=0.5,
                  parents=good, tokens=good, hist=good, seqs=good, scores=good, logp=good, logits=None, ws=good, stream=None)

    def call(form, **over):
        a = dict(common)
        a.update(over)
        head = [ctypes.byref(a['weights']) if a['weights'] is not None else None, a['h0_l0'], a['h0_l1'], a['h0_stride'], a['gib'],
                a['ptab'], a['batch'], a['beats'], a['tpb'], a['hidden'], a['vocab'], a['width']]
        outs = [a['parents'], a['tokens'], a['hist'], a['seqs'], a['scores']]
        tail = [a['logits'], a['ws'], a['stream']]
        plan = None if a['plan'] is None else ctypes.byref(a['plan'])
        if form == 'plain':
            return lib.arvae_tick_beam_search_wide(*head, a['allow'], a['allowed'], *outs, *tail)
        if form == 'planned':
            return lib.arvae_tick_beam_search_wide_planned(*head, plan, *outs, *tail)
        return lib.arvae_tick_beam_search_wide_groups(*head, a['groups'], a['penalty'], plan, *outs, a['logp'], *tail)
    return call


def test_argument_checks_refuse_before_any_launch(lib):
    """every pointer below is a host address that is never dereferenced: each call is refused on the host"""
    from arvae_amd import _lib
    err = lib.arvae_last_error_string
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    good, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    call = _calls(lib, base)
    FORMS = ('plain', 'planned', 'groups')

    def refused(fragment, forms=FORMS, **over):
        for form in forms:
            assert call(form, **over) == -1, (form, over)         # ARVAE_E_INVALID
            assert fragment in err() and b'tick_beam_search_wide' in err(), (form, over, err())

    for missing in ('weights', 'h0_l0', 'h0_l1', 'gib', 'ptab'):
        refused(b'null pointer', **{missing: None})
    for missing in ('parents', 'tokens', 'hist', 'seqs', 'scores'):
        refused(b'null output pointer', **{missing: None})
    refused(b'null log_probs', forms=('groups',), logp=None)
    refused(b'null plan', forms=('planned', 'groups'), plan=None)
    for i, name in enumerate(('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1', 'w_out', 'b_out')):
        if name.startswith('w_'):
            refused(b'16-byte aligned', weights=_lib.TickWeights(*[base + 4 if k == i else base for k in range(8)]))
        refused(b'null weight pointer', weights=_lib.TickWeights(*[None if k == i else base for k in range(8)]))
    refused(b'16-byte aligned', h0_l0=odd)
    refused(b'16-byte aligned', h0_l1=odd)
    refused(b'workspace', ws=None)
    refused(b'workspace', ws=odd)
    for stride in (258, 513, 1, 128):
        refused(b'h0_stride', h0_stride=stride)
    # shapes
    for hid in (64, 128, 384, 100):
        refused(b'not built', hidden=hid)
    for vocab in (1, 129, 0):
        refused(b'vocabulary', vocab=vocab)
    for empty in ('batch', 'beats', 'tpb'):
        refused(b'empty problem', **{empty: 0})
    refused(b'ticks', beats=1 << 20, tpb=1 << 12)               # 2^32 ticks
    refused(b'rows', batch=1 << 28, width=16, groups=4)         # 2^32 rows
    # what the one-launch searches refuse of a width, a mask, a plan and groups
    for width in (0, 17, -3):
        refused(b'[1, 16]', width=width)
    refused(b'width 4 is above the 3 allowed notes', forms=('plain',), allow=good, allowed=3)
    refused(b'without a mask', forms=('plain',), allowed=12)
    refused(b'allowed', forms=('plain',), allow=good, allowed=36)
    refused(b'above the 3 allowed', forms=('plain',), vocab=3, allowed=3)
    refused(b'null plan mask', forms=('planned', 'groups'), plan=_lib.NotePlan(None, 24 * 35, 35))
    refused(b'row stride', forms=('planned', 'groups'), plan=_lib.NotePlan(base, 35, 35))
    refused(b'tick stride', forms=('planned', 'groups'), plan=_lib.NotePlan(base, 24 * 35, 1))
    for groups in (0, 3, 5, -1):
        refused(b'groups', forms=('groups',), groups=groups)
    for penalty in (-0.5, float('inf'), float('nan')):
        refused(b'penalty', forms=('groups',), penalty=penalty)

"""The entry points of the streamed-weights free-running tick decoder (include/arvae_hip.h, arvae_tick_free_run_wide*) without a
GPU: the symbols, what the predicates answer, that every existing predicate keeps its answer, and that every argument check refuses
with its message before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_symbols_and_predicates(lib):
    from arvae_amd import _lib, ops
    assert lib.arvae_abi_version() == _lib.ABI_VERSION == 16   # symbols added, nothing existing changed: the number stays
    for name in ('arvae_tick_free_run_wide_supported', 'arvae_tick_free_run_wide_ws_floats', 'arvae_tick_free_run_wide'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    sup = lib.arvae_tick_free_run_wide_supported
    assert sup(256, 35) == 1 and sup(512, 70) == 1
    assert sup(128, 35) == 0 and sup(384, 35) == 0 and sup(512, 1) == 0
    assert sup(256, 2) == 1 and sup(512, 128) == 1 and sup(512, 129) == 0
    assert ops.tick_free_run_wide_supported(512, 35) and not ops.tick_free_run_wide_supported(128, 35)
    # the one-launch decoders and the resident-weights recurrences answer what they answered
    for hid in (256, 512):
        assert lib.arvae_tick_free_run_supported(hid, 35) == 0 and lib.arvae_gru_seq_supported(hid) == 0
        assert all(lib.arvae_tick_free_run_layers_supported(hid, 35, layers) == 0 for layers in (1, 2, 3, 4))
        assert lib.arvae_tick_beam_search_supported(hid, 35, 4) == 0
    assert lib.arvae_tick_free_run_supported(128, 35) == 1 and lib.arvae_tick_free_run_supported(128, 70) == 0


def test_workspace_size(lib):
    ws = lib.arvae_tick_free_run_wide_ws_floats
    assert ws(0, 256, 35) == -1 and ws(16, 128, 35) == -1 and ws(16, 384, 35) == -1 and ws(16, 256, 1) == -1 and ws(16, 256, 129) == -1
    sizes = [ws(b, 256, 35) for b in (1, 5, 37, 256, 257)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(37, 512, 70) > ws(37, 256, 70)
    assert ws(1 << 22, 512, 35) > 4 * (1 << 22) * 512          # 64-bit


def _args(base, **over):
    """a complete, acceptable argument list whose pointers are host addresses that are never dereferenced -> (list, what keeps it alive)"""
    from arvae_amd import _lib
    good = ctypes.c_void_p(base)
    a = dict(weights=_lib.TickWeights(*[base] * 8), h0_l0=good, h0_l1=good, h0_stride=0, gib=good, ptab=good, mask=None, keep_scale=1.0,
             batch=5, beats=4, tpb=6, hidden=256, vocab=35, uniforms=None, inv_t=1.0, filter=None, plan=None, tokens=good, logits=None,
             ws=good, stream=None)
    a.update(over)
    keep = [a['weights'], a['filter'], a['plan']]
    by = lambda s: None if s is None else ctypes.byref(s)                    # noqa: E731
    return [ctypes.byref(a['weights']), a['h0_l0'], a['h0_l1'], a['h0_stride'], a['gib'], a['ptab'], a['mask'], a['keep_scale'], a['batch'],
            a['beats'], a['tpb'], a['hidden'], a['vocab'], a['uniforms'], a['inv_t'], by(a['filter']), by(a['plan']), a['tokens'],
            a['logits'], a['ws'], a['stream']], keep


def test_argument_checks_refuse_before_any_launch(lib):
    """every pointer below is a host address that is never dereferenced: each call is refused on the host"""
    from arvae_amd import _lib
    fn, err = lib.arvae_tick_free_run_wide, lib.arvae_last_error_string
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    good, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def refused(fragment, **over):
        args, keep = _args(base, **over)
        assert fn(*args) == -1, over                             # ARVAE_E_INVALID
        assert fragment in err(), (over, err())

    flt = _lib.SampleFilter(3, 1.0, None)
    plan = _lib.NotePlan(base, 24 * 35, 35)
    # a keep-mask together with a filter or a plan
    refused(b'keep-mask', mask=good, filter=flt, uniforms=good)
    refused(b'keep-mask', mask=good, filter=flt, plan=plan, uniforms=good)
    # the inverse temperature
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        refused(b'inverse temperature', inv_t=bad)
        refused(b'inverse temperature', inv_t=bad, uniforms=good)
    # 16-byte alignment where the kernels read 16 bytes
    refused(b'workspace', ws=None)
    refused(b'workspace', ws=odd)
    refused(b'16-byte aligned', h0_l0=odd)
    refused(b'16-byte aligned', h0_l1=odd)
    for i, name in enumerate(('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1', 'w_out', 'b_out')):
        if name.startswith('w_'):
            refused(b'16-byte aligned', weights=_lib.TickWeights(*[base + 4 if k == i else base for k in range(8)]))
        refused(b'null weight pointer', weights=_lib.TickWeights(*[None if k == i else base for k in range(8)]))
    # the initial states' row stride
    for stride in (258, 513, 1):
        refused(b'h0_stride', h0_stride=stride)
    refused(b'h0_stride', h0_stride=128)
    # shapes
    for hid in (128, 384, 100):
        refused(b'not built', hidden=hid)
    for vocab in (1, 129):
        refused(b'vocabulary', vocab=vocab)
    for empty in ('batch', 'beats', 'tpb'):
        refused(b'empty problem', **{empty: 0})
    for missing in ('h0_l0', 'h0_l1', 'gib', 'ptab', 'tokens'):
        refused(b'null pointer', **{missing: None})
    # what the filtered and the planned row entry points refuse
    refused(b'null uniforms', filter=flt)
    refused(b'null uniforms', filter=flt, plan=plan)
    refused(b'null filter', plan=plan, uniforms=good)
    refused(b'top_k', filter=_lib.SampleFilter(36, 1.0, None), uniforms=good)
    refused(b'top_p', filter=_lib.SampleFilter(0, 0.0, None), uniforms=good)
    refused(b'filter->allow', filter=_lib.SampleFilter(3, 1.0, base), plan=plan, uniforms=good)
    refused(b'null plan mask', filter=flt, plan=_lib.NotePlan(None, 24 * 35, 35), uniforms=good)
    refused(b'row stride', filter=flt, plan=_lib.NotePlan(base, 35, 35), uniforms=good)
    refused(b'tick stride', filter=flt, plan=_lib.NotePlan(base, 24 * 35, 1), uniforms=good)

"""The entry points of the streamed-weights GRU recurrences (include/arvae_hip.h, arvae_gru_seq_wide_*) without a GPU: what the
predicates answer, that the resident-weights predicates and everything derived from them keep their meaning at 256 and 512, and
that every argument check refuses with its message before anything is launched."""
import ctypes

import pytest
import torch

from arvae_amd import synthetic as syn


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


class _FolkDataset:
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


def test_predicates(lib):
    from arvae_amd import ops
    from arvae_amd import _lib
    assert lib.arvae_abi_version() == _lib.ABI_VERSION        # symbols added, nothing existing changed: the number stays
    assert all(hasattr(lib, 'arvae_gru_seq_wide_' + n) and 'arvae_gru_seq_wide_' + n in _lib.SIGNATURES for n in ('supported', 'ws_floats', 'fwd', 'bwd'))
    assert lib.arvae_gru_seq_wide_supported(256) == 1 and lib.arvae_gru_seq_wide_supported(512) == 1
    assert lib.arvae_gru_seq_wide_supported(128) == 0 and lib.arvae_gru_seq_wide_supported(384) == 0
    assert ops.gru_sequence_wide_supported(512) and not ops.gru_sequence_wide_supported(128)
    # "the resident-weights kernels": unchanged, and so is every one-launch decoder derived from it
    assert lib.arvae_gru_seq_supported(256) == 0 and lib.arvae_gru_seq_supported(512) == 0
    assert not ops.gru_sequence_supported(256) and ops.gru_sequence_supported(128)
    vocab = len(_FolkDataset().note2index_dicts)
    assert vocab == 35
    for hid in (256, 512):
        assert lib.arvae_tick_free_run_supported(hid, vocab) == 0
        assert all(lib.arvae_tick_free_run_layers_supported(hid, vocab, layers) == 0 for layers in (1, 2, 3, 4))
        assert all(lib.arvae_tick_beam_search_supported(hid, vocab, width) == 0 for width in (1, 4, 16))
        assert lib.arvae_tick_beam_search_groups_supported(hid, vocab, 4, 2) == 0


def test_sequence_path_is_chosen_at_the_wide_sizes(lib, monkeypatch):
    from arvae_amd import measure_vae
    monkeypatch.delenv('ARVAE_GRU_STEPWISE', raising=False)
    assert all(measure_vae._use_sequence_kernels(h) for h in (32, 64, 128, 256, 512))
    assert not measure_vae._use_sequence_kernels(384) and not measure_vae._use_sequence_kernels(100)
    monkeypatch.setenv('ARVAE_GRU_STEPWISE', '1')
    assert not any(measure_vae._use_sequence_kernels(h) for h in (128, 256, 512))


def test_executor_still_declines_a_wide_model(lib):
    from arvae_amd.fused_measure import FusedMeasureVAE
    from arvae_amd.measure_vae import MeasureVAE
    model = MeasureVAE(_FolkDataset(), 10, 2, 2, 256, 0.5, 32, 2, 256, 0.5, False, 'folk')
    assert FusedMeasureVAE.supports(model, None, (0, 1, 2, 3)) == 'hidden size not built as a sequence kernel'


def test_workspace_size(lib):
    ws = lib.arvae_gru_seq_wide_ws_floats
    assert ws(0, 16, 256) == -1 and ws(5, 16, 256) == -1 and ws(1, 0, 256) == -1 and ws(1, 16, 128) == -1 and ws(1, 16, 384) == -1
    a, b = ws(2, 37, 256), ws(2, 74, 256)
    assert a > 0 and b == 2 * a and a % 4 == 0                 # two carried-gradient buffers of nseq x rows x hidden
    assert ws(4, 37, 256) == 2 * a and ws(2, 37, 512) == 2 * a
    assert ws(4, 1 << 20, 512) == 2 * 4 * (1 << 20) * 512      # 64-bit


def _descs(n, fields):
    from arvae_amd import _lib
    seqs = (_lib.GruSeqDesc * n)()
    for q in seqs:
        for name, value in fields.items():
            setattr(q, name, value)
    return seqs


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_argument_checks_refuse_before_any_launch(lib, which):
    """every pointer below is a host address that is never dereferenced: each call is refused on the host"""
    fn = getattr(lib, 'arvae_gru_seq_wide_' + which)
    err = lib.arvae_last_error_string
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    good = ctypes.c_void_p(base)
    every = dict(gi=base, w_hh=base, b_hh=base, h_all=base, saved=base, dgi=base, dgh=base, h_stride=256)
    seqs = _descs(1, every)
    assert fn(None, 1, 6, 16, 256, good, None) == -1 and b'sequences per call' in err()
    for nseq in (0, 5):
        assert fn(_descs(max(nseq, 1), every), nseq, 6, 16, 256, good, None) == -1 and b'1..4 sequences' in err()
    assert fn(seqs, 1, 0, 16, 256, good, None) == -1 and b'empty sequence' in err()
    assert fn(seqs, 1, 6, 0, 256, good, None) == -1 and b'empty sequence' in err()
    for hid in (128, 384, 100):
        assert fn(seqs, 1, 6, 16, hid, good, None) == -1 and b'hidden size' in err() and b'not built' in err()
    assert fn(seqs, 1, 6, 16, 256, None, None) == -1 and b'workspace' in err()
    assert fn(seqs, 1, 6, 16, 256, ctypes.c_void_p(base + 4), None) == -1 and b'workspace' in err()
    for missing in (('gi', 'b_hh', 'w_hh', 'h_all', 'saved') if which == 'fwd' else ('w_hh', 'h_all', 'saved', 'dgi', 'dgh')):
        assert fn(_descs(1, {k: v for k, v in every.items() if k != missing}), 1, 6, 16, 256, good, None) == -1 and b'null pointer' in err(), missing
    misaligned = dict(every, **({'w_hh': base + 4} if which == 'fwd' else {'dgh': base + 4}))
    assert fn(_descs(1, misaligned), 1, 6, 16, 256, good, None) == -1 and b'16-byte aligned' in err()
    assert fn(_descs(1, dict(every, h_stride=128)), 1, 6, 16, 256, good, None) == -1 and b'h_stride' in err()


def test_resident_entry_points_still_refuse_the_wide_sizes(lib):
    seqs = _descs(1, {})
    assert lib.arvae_gru_seq_fwd(seqs, 1, 24, 16, 256, None) == -1 and b'hidden size 256 is not built' in lib.arvae_last_error_string()
    assert lib.arvae_gru_seq_bwd(seqs, 1, 24, 16, 512, None) == -1 and b'hidden size 512 is not built' in lib.arvae_last_error_string()

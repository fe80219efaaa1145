"""Top-k, nucleus (top-p) and note-mask sampling of the free-running decoder, host side: the float64 restatement of the semantics
(include/arvae_hip.h, arvae_sample_filter_t; the yardstick of tests/test_sampling_filters_gpu.py), the three entry points' argument
validation and the struct's layout without a GPU, and the host-side checks of generate / sample_measures / the command line."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import arvae_amd  # noqa: F401
from arvae_amd import _lib
from arvae_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampling import _FolkDataset, pick64  # noqa: E402


# ---------------------------------------------------------------- the semantics, in float64
def order64(logits, allow=None):
    """-> (order (..., V): the notes by descending logit, ties to the lower index, the banned ones last; allowed (..., V) bool)"""
    l = np.asarray(logits, np.float64)
    a = np.ones(l.shape, bool) if allow is None else np.broadcast_to(np.asarray(allow).astype(bool), l.shape)
    return np.argsort(-np.where(a, l, -np.inf), axis=-1, kind='stable'), a


def filter64(logits, allow, top_k, top_p, tau, details=False):
    """the keep-set (..., V) bool: v is allowed, rank(v) < top_k (0 / None: off), mass_before(v) < top_p (1 / None: off; the first
    note of the order always survives).  details: also (order, sorted logits, sorted allowed flags, mass_before in sorted order)"""
    l = np.asarray(logits, np.float64)
    v = l.shape[-1]
    order, a = order64(l, allow)
    ls, as_ = np.take_along_axis(l, order, -1), np.take_along_axis(a, order, -1)
    k = v if not top_k else int(top_k)
    in_k = as_ & (np.arange(v) < k)
    e = np.where(as_, np.exp((ls - ls[..., :1]) / tau), 0.0)             # (the first of the order holds the allowed maximum)
    s = np.where(in_k, e, 0.0).sum(-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        before = (np.cumsum(e, -1) - e) / s
    keep_sorted = in_k.copy()
    if top_p is not None and top_p < 1.0:
        keep_sorted &= before < top_p
    keep_sorted[..., 0] = as_[..., 0]
    keep = np.zeros(l.shape, bool)
    np.put_along_axis(keep, order, keep_sorted, -1)
    return (keep, order, ls, as_, before) if details else keep


def pick64_filtered(logits, u, tau, allow=None, top_k=0, top_p=1.0):
    """-> (token, distance of u to the nearest bracket boundary): test_sampling.pick64 over the survivors (the cut notes weigh 0)"""
    keep = filter64(logits, allow, top_k, top_p, tau)
    return pick64(np.where(keep, np.asarray(logits, np.float64), -np.inf), u, tau)


def test_float64_filter_restates_the_semantics():
    l = np.array([0.0, 3.0, 0.0, 1.0, 0.0, 2.0])
    # the order: 1 (3.0), 5 (2.0), 3 (1.0), then the ties at logit 0 by index
    np.testing.assert_array_equal(order64(l)[0], [1, 5, 3, 0, 2, 4])
    for k, want in ((1, [1]), (2, [1, 5]), (4, [0, 1, 3, 5]), (5, [0, 1, 2, 3, 5]), (6, range(6)), (0, range(6))):
        np.testing.assert_array_equal(np.flatnonzero(filter64(l, None, k, 1.0, 1.0)), sorted(want))
    # top_k = 1 is the argmax, lowest index on ties, at every draw
    for row in (l, np.zeros(5), np.array([0.0, 2.0, 2.0])):
        for u in (2.0 ** -32, 0.3, 1.0):
            assert pick64_filtered(row, u, 1.0, top_k=1)[0] == int(np.argmax(row))
    # top_p: mass_before over S; the first note survives even when its mass alone exceeds p
    e = np.exp(np.sort(l)[::-1] - 3.0)
    before = (np.cumsum(e) - e) / e.sum()
    for p in (0.05, 0.5, 0.7, 0.9, 0.97):
        want = np.array([1, 5, 3, 0, 2, 4])[before < p]
        np.testing.assert_array_equal(np.flatnonzero(filter64(l, None, 0, p, 1.0)), sorted(want))
    assert e[0] / e.sum() > 0.5 and filter64(l, None, 0, 0.05, 1.0).sum() == 1
    # S is the mass top_k leaves: with top_k = 2 note 5's mass_before is e0 / (e0 + e1) = 0.731
    assert filter64(l, None, 2, 0.72, 1.0).sum() == 1 and filter64(l, None, 2, 0.74, 1.0).sum() == 2
    # the temperature moves the nucleus
    assert filter64(l, None, 0, 0.7, 2.0).sum() > filter64(l, None, 0, 0.7, 0.5).sum()
    # nothing active: pick64 itself
    rs = np.random.RandomState(0)
    rows = np.maximum(rs.normal(size=(50, 35)) * 2.0, 0.0)
    u = 1.0 - rs.random_sample(50)
    for kw in ({}, {'top_k': 35}, {'top_k': 0, 'top_p': 1.0}, {'allow': np.ones(35, np.uint8)}):
        np.testing.assert_array_equal(pick64_filtered(rows, u, 0.8, **kw)[0], pick64(rows, u, 0.8)[0])
    # the mask comes first: ranks are taken among the allowed notes, the maximum too
    allow = np.array([1, 0, 1, 1, 1, 0], np.uint8)
    np.testing.assert_array_equal(np.flatnonzero(filter64(l, allow, 2, 1.0, 1.0)), [0, 3])
    np.testing.assert_array_equal(np.flatnonzero(filter64(l, allow, 0, 1.0, 1.0)), [0, 2, 3, 4])
    assert pick64_filtered(l, 1.0, 1.0, allow=allow, top_k=1)[0] == 3
    one = np.zeros(6, np.uint8)
    one[4] = 1
    assert all(pick64_filtered(l, u, 1.0, allow=one, top_p=0.3)[0] == 4 for u in (2.0 ** -32, 0.5, 1.0))
    # the draw runs over the survivors in index order
    keep = filter64(l, None, 3, 1.0, 1.0)                                 # notes 1, 3, 5 with e = 1, e^-2, e^-1
    c = np.cumsum(np.where(keep, np.exp(l - 3.0), 0.0))
    c /= c[-1]
    assert pick64_filtered(l, c[1], 1.0, top_k=3)[0] == 1 and pick64_filtered(l, c[1] + 1e-9, 1.0, top_k=3)[0] == 3
    assert pick64_filtered(l, c[3] + 1e-9, 1.0, top_k=3)[0] == 5 and pick64_filtered(l, 1.0, 1.0, top_k=3)[0] == 5


# ---------------------------------------------------------------- the cases of the row sampler's device test, and their float64 side
ROW_COLS = (1, 16, 35, 64, 200)
ROW_PARAMS = ((0, 1.0, 1.0), (1, 1.0, 1.0), (5, 1.0, 1.0), (0, 0.8, 1.0), (8, 0.6, 1.0))     # (top_k, top_p, tau)
ROW_ROWS = 257
DELTA_ROW = 1e-5                                                          # tests/test_sampling_gpu.py's


def row_case(cols, top_k, top_p, masked):
    """(logits float32 (257, cols) = relu(N(0, 2)), u float32 (257,) in (0, 1], allow uint8 (cols,) or None, top_k clipped to cols)"""
    rs = np.random.RandomState(1000 * cols + 10 * top_k + int(100 * top_p) + int(masked))
    logits = np.maximum(rs.normal(size=(ROW_ROWS, cols)) * 2.0, 0.0).astype(np.float32)
    u = np.clip((1.0 - rs.random_sample(ROW_ROWS)).astype(np.float32), np.float32(2.0 ** -32), np.float32(1.0))
    u[:2] = [1.0, 2.0 ** -32]
    allow = None
    if masked:
        allow = np.zeros(cols, np.uint8)
        allow[rs.permutation(cols)[:max(1, cols // 2)]] = 1
    return logits, u, allow, min(top_k, cols)


def check_row_picks(tokens, logits, u, tau, allow, top_k, top_p, delta):
    """clear draws equal the float64 pick; a draw is ambiguous when some mass_before lies within delta of top_p or u within delta of
    a bracket boundary, and must then come from the keep-set at top_p + delta.  -> the ambiguous share"""
    tokens = np.asarray(tokens)
    keep, _, _, as_, before = filter64(logits, allow, top_k, top_p, tau, details=True)
    want, dist = pick64_filtered(logits, u, tau, allow, top_k, top_p)
    v = keep.shape[-1]
    in_k = as_ & (np.arange(v) < (top_k or v))
    near_p = (in_k & (np.abs(before - top_p) <= delta)).any(-1) if top_p < 1.0 else np.zeros(len(tokens), bool)
    clear = ~near_p & (dist > delta)
    assert tokens.min() >= 0 and tokens.max() < v
    np.testing.assert_array_equal(tokens[clear], want[clear])
    wide = filter64(logits, allow, top_k, min(top_p + delta, 1.0), tau)
    assert np.take_along_axis(wide, tokens[:, None], -1).all()
    return 1.0 - clear.mean()


@pytest.mark.parametrize('cols', ROW_COLS)
def test_row_cases_are_rarely_ambiguous_in_float64(cols):
    """the float64 restatement alone: the share of draws the band rule exempts is of order cols * 2e-5, far below the 0.05 cap of
    the device test, and the picks satisfy their own check"""
    for top_k, top_p, tau in ROW_PARAMS:
        for masked in (False, True):
            logits, u, allow, k = row_case(cols, top_k, top_p, masked)
            want = pick64_filtered(logits, u, tau, allow, k, top_p)[0]
            share = check_row_picks(want, logits, u, tau, allow, k, top_p, DELTA_ROW)
            assert share <= 0.02, (cols, top_k, top_p, masked, share)
            if allow is not None:
                assert allow[want].all()


def check_tick_picks(tokens, weights, u, tau, allow, top_k, top_p, eps, delta):
    """picks against weights known to eps (the whole-sequence kernels' against the tick kernel's own logits).  A draw is ambiguous when
    u lies within delta of a bracket boundary, the top_k-th and (top_k+1)-th ordered logits lie within 2 eps, some mass_before lies
    within delta of top_p, or the last note the cuts keep and the first they drop lie within 2 eps.  The last criterion is the
    top_k one applied to the cut that is actually in force: when the nucleus ends before top_k does, two logits within 2 eps on
    either side of ITS edge may stand in the other order in the kernel's own logits (each is known to eps only), which swaps a
    kept note for a dropped one although every mass_before is far from top_p -- a mass_before moves by a whole e_v when v changes
    places, not by delta.  Without it such a draw would be called clear and compared with a pick the data cannot decide; the
    0.05 cap on the ambiguous share covers it like the others.  Clear draws equal the float64 pick; ambiguous ones are allowed
    notes of the keep-set at top_k + 1 and top_p + delta.  -> (ambiguous share, clear (B, T) bool)"""
    tokens = np.asarray(tokens)
    w = np.asarray(weights, np.float64)
    v = w.shape[-1]
    keep, _, ls, as_, before = filter64(w, allow, top_k, top_p, tau, details=True)
    want, dist = pick64_filtered(w, u, tau, allow, top_k, top_p)
    k = top_k or v
    in_k = as_ & (np.arange(v) < k)
    amb = dist <= delta
    if k < v:
        amb |= as_[..., k] & (np.abs(ls[..., k - 1] - ls[..., k]) <= 2.0 * eps)
    if top_p < 1.0:
        amb |= (in_k & (np.abs(before - top_p) <= delta)).any(-1)
    n_keep = keep.sum(-1)                                                 # the survivors are a leading run of the order
    nxt = np.minimum(n_keep, v - 1)
    last = np.take_along_axis(ls, np.maximum(n_keep - 1, 0)[..., None], -1)[..., 0]
    first_cut = np.take_along_axis(ls, nxt[..., None], -1)[..., 0]
    amb |= (n_keep < v) & np.take_along_axis(as_, nxt[..., None], -1)[..., 0] & (np.abs(last - first_cut) <= 2.0 * eps)
    clear = ~amb
    assert tokens.min() >= 0 and tokens.max() < v
    np.testing.assert_array_equal(tokens[clear], want[clear])
    wide = filter64(w, allow, min(k + 1, v), min(top_p + delta, 1.0), tau)
    ok = np.take_along_axis(wide, tokens[..., None], -1)[..., 0]
    assert ok.all(), (tokens[~ok][:8], want[~ok][:8])
    return 1.0 - clear.mean(), clear


# ---------------------------------------------------------------- the library's entry points without a GPU
@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _err(lib):
    return lib.arvae_last_error_string().decode()


BAD_FILTERS = [((-1, 1.0), 'top_k'), ((36, 1.0), 'top_k'), ((0, 0.0), 'top_p'), ((0, -0.5), 'top_p'), ((0, 1.5), 'top_p'),
               ((0, math.nan), 'top_p'), ((0, math.inf), 'top_p')]


def test_row_sample_filtered_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 70)()
    idx = (ctypes.c_int64 * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def call(top_k=3, top_p=0.9, allow=None, w=p(buf), u=p(buf), inv_t=1.0, out=p(idx), cols=35, flt=True):
        f = _lib.SampleFilter(top_k, top_p, allow)
        return lib.arvae_row_sample_filtered(w, 2, cols, u, inv_t, ctypes.byref(f) if flt else None, out, None)
    for (k, pp), word in BAD_FILTERS:
        assert call(k, pp) == -1 and 'row_sample_filtered' in _err(lib) and word in _err(lib), (k, pp)
    assert call(flt=False) == -1 and 'null filter' in _err(lib)
    assert call(u=None) == -1 and 'null uniforms' in _err(lib)
    assert call(w=None) == -1 and call(out=None) == -1
    assert call(cols=0, top_k=0) == -1
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert call(inv_t=bad) == -1 and 'inverse temperature' in _err(lib)
        assert call(top_k=0, top_p=1.0, inv_t=bad) == -1 and 'inverse temperature' in _err(lib)     # (forwarded to arvae_row_sample)


def test_tick_free_run_filtered_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    tok = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    tw = _lib.TickWeights(*([p] * 8))

    def call(top_k=3, top_p=0.9, allow=None, uniforms=p, inv_t=1.0, ws=p, hidden=128, vocab=35, mask=None, flt=True):
        f = _lib.SampleFilter(top_k, top_p, allow)
        return lib.arvae_tick_free_run_filtered(ctypes.byref(tw), p, p, 0, p, p, mask, 1.0, 1, 4, 6, hidden, vocab, uniforms, inv_t,
                                                ctypes.byref(f) if flt else None, ctypes.cast(tok, ctypes.c_void_p), ws, None)
    for (k, pp), word in BAD_FILTERS:
        assert call(k, pp) == -1 and 'tick_free_run_filtered' in _err(lib) and word in _err(lib), (k, pp)
    assert call(flt=False) == -1 and 'null filter' in _err(lib)
    assert call(uniforms=None) == -1 and 'null uniforms' in _err(lib)
    assert call(mask=p) == -1 and 'dropout' in _err(lib)
    assert call(top_k=0, top_p=1.0, mask=p) == -1 and 'dropout' in _err(lib)          # also when nothing is active
    assert call(ws=None) == -1 and 'workspace' in _err(lib)
    assert call(top_k=0, top_p=1.0, ws=None) == -1 and 'workspace' in _err(lib)
    for bad in (0.0, -1.0, math.nan):
        assert call(inv_t=bad) == -1 and 'inverse temperature' in _err(lib)
    assert call(hidden=48) == -1 and call(vocab=65, top_k=0) == -1 and call(hidden=32, vocab=35) == -1    # as arvae_tick_free_run


def test_tick_free_run_layers_filtered_rejects_bad_arguments(lib):
    p = ctypes.c_void_p(256)                                   # never dereferenced: every call below fails validation first
    tok = (ctypes.c_int64 * 24)()

    def stack(layers):
        s = _lib.TickStack()
        s.layers = layers
        for l in range(min(layers, 4)):
            s.w_ih[l], s.w_hh[l], s.b_ih[l], s.b_hh[l], s.h0[l] = 256, 256, 256, 256, 256
        s.w_out, s.b_out = 256, 256
        return s

    def call(s, top_k=3, top_p=0.9, uniforms=p, inv_t=1.0, ws=p, hidden=64, vocab=35, mask=None, flt=True):
        f = _lib.SampleFilter(top_k, top_p, None)
        return lib.arvae_tick_free_run_layers_filtered(ctypes.byref(s), p, p, mask, 1.0, 1, 4, 6, hidden, vocab, uniforms, inv_t,
                                                       ctypes.byref(f) if flt else None, ctypes.cast(tok, ctypes.c_void_p), ws, None)
    for (k, pp), word in BAD_FILTERS:
        assert call(stack(3), k, pp) == -1 and 'tick_free_run_layers_filtered' in _err(lib) and word in _err(lib), (k, pp)
    assert call(stack(3), flt=False) == -1 and 'null filter' in _err(lib)
    assert call(stack(3), uniforms=None) == -1 and 'null uniforms' in _err(lib)
    assert call(stack(3), mask=p) == -1 and 'dropout' in _err(lib)
    assert call(stack(3), ws=None) == -1 and 'workspace' in _err(lib)
    assert call(stack(2)) == -1 and 'arvae_tick_free_run' in _err(lib)               # the supported shapes are the unfiltered call's
    assert call(stack(3), hidden=128) == -1 and 'not offered' in _err(lib)
    assert call(stack(1), hidden=32, vocab=35, top_k=0) == -1 and 'vocabulary' in _err(lib)
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert call(stack(3), inv_t=bad) == -1 and 'temperature' in _err(lib)


def test_sample_filter_struct_matches_the_header(tmp_path):
    """sizeof / field offsets of arvae_sample_filter_t as gcc lays it out == the ctypes mirror"""
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('gcc not available')
    fields = ['top_k', 'top_p', 'allow']
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/arvae_hip.h"', 'int main(void) {',
             r'printf("%zu %d\n", sizeof(arvae_sample_filter_t), ARVAE_ABI_VERSION);']
    lines += [rf'printf("%zu\n", offsetof(arvae_sample_filter_t, {f}));' for f in fields] + ['return 0; }']
    src = tmp_path / 'sizes.c'
    src.write_text('\n'.join(lines))
    subprocess.run([gcc, '-o', str(tmp_path / 'sizes'), str(src)], check=True)
    out = subprocess.run([str(tmp_path / 'sizes')], check=True, capture_output=True, text=True).stdout.split()
    assert [int(out[0]), int(out[1])] == [ctypes.sizeof(_lib.SampleFilter), _lib.ABI_VERSION]
    assert [int(v) for v in out[2:]] == [getattr(_lib.SampleFilter, f).offset for f in fields]


# ---------------------------------------------------------------- the host side of generate / sample_measures / the command line
def _model_and_trainer():
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    torch.manual_seed(0)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.5, 16, 2, 64, 0.5, False, 'folk')
    return ds, model, MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))


def test_generate_validates_its_cuts_on_the_host():
    _, model, _ = _model_and_trainer()
    dec = model.decoder
    z = torch.zeros(3, 16)
    for kw in ({'top_k': 0}, {'top_k': 36}, {'top_k': -2}, {'top_p': 0.0}, {'top_p': 1.01}, {'top_p': float('nan')}, {'top_p': -0.1},
               {'allowed': np.zeros(35, np.uint8)}, {'allowed': np.ones(34, np.uint8)}, {'allowed': np.ones((35, 1), bool)},
               {'allowed': np.full(35, 2, np.uint8)}):
        with pytest.raises(ValueError):
            dec.generate(z, **kw)
    for kw in ({'top_k': 2.5}, {'top_k': True}, {'top_k': '3'}, {'top_p': '0.5'}, {'top_p': None, 'top_k': None, 'allowed': np.ones(35, np.float32)}):
        with pytest.raises(TypeError):
            dec.generate(z, **kw)
    with pytest.raises(ValueError, match='multinomial'):
        dec.generate(z, sampling='argmax', top_k=3)
    assert dec.sampling_filter() is None
    k, p, allow = dec.sampling_filter(np.int64(5), 1, [True] * 3 + [False] * 32)
    assert (k, p) == (5, 1.0) and type(k) is int and type(p) is float
    assert allow.dtype == torch.uint8 and allow.tolist() == [1] * 3 + [0] * 32
    # valid cuts get as far as the device: what is missing here is the GPU, and the decoder is left as it was
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec.generate(z, top_k=4, top_p=0.9, allowed=torch.ones(35, dtype=torch.bool))
    assert dec._filter is None and dec.sampling == 'argmax' and dec.use_teacher_forcing is True and dec.temperature == 1.0


def test_playable_mask_and_sample_measures_arguments():
    ds, _, trainer = _model_and_trainer()
    names = ds.index2note_dicts
    mask = trainer.playable_mask()
    assert mask.dtype == torch.uint8 and mask.shape == (35,)
    banned = {names[i] for i in range(35) if not mask[i]}
    assert banned == {'START', 'END', None} and int(mask.sum()) == 32
    assert mask[ds.note2index_dicts['__']] == 1 and mask[ds.note2index_dicts['rest']] == 1       # the slur and the rest are music
    only = np.zeros(35, np.uint8)
    only[[ds.note2index_dicts['START'], ds.note2index_dicts['rest'], 20]] = 1
    both = trainer.playable_mask(only)
    assert sorted(np.flatnonzero(both.numpy())) == sorted([ds.note2index_dicts['rest'], 20])
    # a vocabulary of its own
    class Tiny:
        index2note_dicts = {0: 'C4', 1: 'END', 2: None, 3: '__', 4: 'START', 5: 'rest', 6: 'D4'}
    trainer.dataset = Tiny()
    assert trainer.playable_mask().tolist() == [1, 0, 0, 1, 0, 1, 1]
    trainer.dataset = ds
    for kw in ({'top_k': 0}, {'top_k': 99}, {'top_p': 0.0}, {'top_p': 2.0}, {'allowed': np.zeros(35, np.uint8)}):
        with pytest.raises(ValueError):
            trainer.sample_measures(4, **kw)
        with pytest.raises(ValueError):
            trainer.decode_latent_codes(torch.zeros(2, 16), sampling='multinomial', **kw)
    pads = np.zeros(35, np.uint8)
    pads[[ds.note2index_dicts['START'], ds.note2index_dicts['END']]] = 1
    with pytest.raises(ValueError, match='allows no note'):                   # nothing is left once the padding symbols go
        trainer.sample_measures(4, allowed=pads, playable=True)


def test_cli_rejects_bad_cuts(monkeypatch):
    sys.path.insert(0, ROOT)
    import train_measure_vae as cli
    for args in (['--sample', '2', '--top_k', '0'], ['--sample', '2', '--top_p', '0'], ['--sample', '2', '--top_p', '1.5'],
                 ['--sample', '2', '--top_p', 'nan'], ['--top_k=-3']):
        with pytest.raises(ValueError):
            cli.run(args)
    assert '--top_k' in cli.SAMPLE_HELP and '--top_p' in cli.SAMPLE_HELP and '--playable' in cli.SAMPLE_HELP

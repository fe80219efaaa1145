"""Multinomial feedback of the hierarchical decoder (measurevae/decoder.py:372,431-434,502-505), host side: the float64 picker that
restates the sampling semantics (the yardstick of tests/test_sampling_gpu.py), the new entry points' argument validation without
a GPU, and the decoder's `sampling` attribute."""
import ctypes
import math

import numpy as np
import pytest
import torch

import arvae_amd  # noqa: F401
from arvae_amd import _lib
from arvae_amd import synthetic as syn


# ---------------------------------------------------------------- the semantics, in float64
def cdf64(logits, tau):
    """normalised CDF (..., V) of softmax(logits / tau): e_v = exp((l_v - max l) / tau), C_k = sum_{v <= k} e_v, C_k / C_{V-1}"""
    l = np.asarray(logits, np.float64)
    c = np.cumsum(np.exp((l - l.max(-1, keepdims=True)) / tau), -1)
    return c / c[..., -1:]


def pick64(logits, u, tau):
    """-> (token = the smallest k with C_k >= u * C_{V-1}, distance of u to the nearest inner bracket boundary C_k / C_{V-1}, k < V - 1)"""
    cdf = cdf64(logits, tau)
    u = np.asarray(u, np.float64)[..., None]
    tok = (cdf[..., :-1] < u).sum(-1)                    # (the last prefix is the total: never below u <= 1)
    dist = np.abs(cdf[..., :-1] - u).min(-1) if cdf.shape[-1] > 1 else np.full(tok.shape, np.inf)
    return tok, dist


def check_picks(tokens, logits, u, tau, delta):
    """the band rule: a token equals the float64 pick wherever u is farther than delta from every float64 bracket boundary; inside
    that band it may be either neighbour of the boundary, i.e. u lies in the token's own bracket widened by delta.
    -> fraction of draws inside the band"""
    tokens = np.asarray(tokens)
    want, dist = pick64(logits, u, tau)
    cdf = cdf64(logits, tau)
    v = cdf.shape[-1]
    assert tokens.min() >= 0 and tokens.max() < v
    clear = dist > delta
    np.testing.assert_array_equal(tokens[clear], want[clear])
    u = np.asarray(u, np.float64)
    upper = np.take_along_axis(cdf, tokens[..., None], -1)[..., 0]
    lower = np.where(tokens > 0, np.take_along_axis(cdf, np.maximum(tokens - 1, 0)[..., None], -1)[..., 0], 0.0)
    ok = (u > lower - delta) & (u <= upper + delta)
    assert ok.all(), (tokens[~ok][:8], want[~ok][:8], u[~ok][:8])
    return 1.0 - clear.mean()


def chi_square(tokens, logits, tau):
    """Pearson chi-square of the token counts against the float64 softmax over the bins with expectation >= 5 -> (value, bins)"""
    l = np.asarray(logits, np.float64)
    p = np.exp((l - l.max()) / tau)
    p /= p.sum()
    expect = len(tokens) * p
    keep = expect >= 5
    obs = np.bincount(np.asarray(tokens).ravel(), minlength=len(p))
    return float(((obs[keep] - expect[keep]) ** 2 / expect[keep]).sum()), int(keep.sum())


def test_float64_picker_restates_the_semantics():
    l = np.array([0.0, 1.0, 0.0, 2.0])
    e = np.exp(l - 2.0)
    cdf = np.cumsum(e) / e.sum()
    for k in range(4):
        lo = cdf[k - 1] if k else 0.0
        assert pick64(l, np.float64(lo + 1e-9), 1.0)[0] == k and pick64(l, cdf[k], 1.0)[0] == k      # (lo, C_k] -> k
    assert pick64(l, 1.0, 1.0)[0] == 3 and pick64(l, 2.0 ** -32, 1.0)[0] == 0
    zeros = np.zeros(35)
    u = np.array([2.0 ** -32, 0.5, 1.0, 1.0 / 35, 1.0 / 35 + 1e-9])
    np.testing.assert_array_equal(pick64(zeros[None].repeat(5, 0), u, 1.0)[0], np.ceil(u * 35 - 1e-12).astype(int) - 1)
    big = np.zeros(35)
    big[17] = 1e4                                             # the maximum is subtracted: no overflow, every draw lands on it
    assert pick64(big, 2.0 ** -32, 1.0)[0] == 17 and pick64(big, 1.0, 1.0)[0] == 17
    tok, dist = pick64(l, cdf[1] + 3e-6, 1.0)
    assert tok == 2 and dist == pytest.approx(3e-6, rel=1e-3)
    assert check_picks(np.array([1]), l[None], np.array([cdf[1] + 3e-6]), 1.0, 1e-5) == 1.0          # in the band: either neighbour
    with pytest.raises(AssertionError):
        check_picks(np.array([1]), l[None], np.array([cdf[1] + 3e-5]), 1.0, 1e-5)
    # the temperature flattens (tau > 1) or sharpens (tau < 1) the distribution
    assert cdf64(l, 2.0)[0] > cdf64(l, 1.0)[0] > cdf64(l, 0.5)[0]
    assert chi_square(np.repeat(np.arange(4), [10, 20, 10, 60]), np.log([1.0, 2.0, 1.0, 6.0]), 1.0) == (pytest.approx(0.0, abs=1e-9), 4)


# ---------------------------------------------------------------- the library's entry points without a GPU
@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _err(lib):
    return lib.arvae_last_error_string().decode()


def test_row_sample_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 8)()
    idx = (ctypes.c_int64 * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.arvae_row_sample(None, 2, 4, p(buf), 1.0, p(idx), None) == -1
    assert lib.arvae_row_sample(p(buf), 2, 4, None, 1.0, p(idx), None) == -1
    assert lib.arvae_row_sample(p(buf), 2, 4, p(buf), 1.0, None, None) == -1
    assert lib.arvae_row_sample(p(buf), 2, 0, p(buf), 1.0, p(idx), None) == -1
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.arvae_row_sample(p(buf), 2, 4, p(buf), bad, p(idx), None) == -1
        assert 'row_sample: inverse temperature' in _err(lib)


def test_philox_uniform_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 8)()
    assert lib.arvae_philox_uniform(None, 8, 1, 0, 0, None, None) == -1
    assert lib.arvae_philox_uniform(ctypes.cast(buf, ctypes.c_void_p), 0, 1, 0, 0, None, None) == -1
    assert 'philox_uniform' in _err(lib)


def test_tick_free_run_sampled_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    tok = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    tw = _lib.TickWeights(*([p] * 8))

    def call(uniforms=p, inv_t=1.0, ws=p, hidden=128, vocab=35):
        return lib.arvae_tick_free_run_sampled(ctypes.byref(tw), p, p, 0, p, p, None, 1.0, 1, 4, 6, hidden, vocab, uniforms, inv_t,
                                               ctypes.cast(tok, ctypes.c_void_p), ws, None)
    assert call(uniforms=None) == -1 and 'null uniforms' in _err(lib)
    assert call(ws=None) == -1 and 'workspace' in _err(lib)
    assert lib.arvae_tick_free_run(ctypes.byref(tw), p, p, 0, p, p, None, 1.0, 1, 4, 6, 128, 35, ctypes.cast(tok, ctypes.c_void_p), None,
                                   None) == -1 and 'workspace' in _err(lib)     # the argmax pass needs it as well
    for bad in (0.0, -1.0, math.nan):
        assert call(inv_t=bad) == -1 and 'inverse temperature' in _err(lib)
    assert call(hidden=48) == -1 and call(vocab=65) == -1 and call(hidden=32, vocab=35) == -1       # as arvae_tick_free_run
    assert lib.arvae_tick_free_run_sampled(None, p, p, 0, p, p, None, 1.0, 1, 4, 6, 128, 35, p, 1.0, ctypes.cast(tok, ctypes.c_void_p), p,
                                           None) == -1


# ---------------------------------------------------------------- the decoder's attribute
class _FolkDataset:
    """the attributes MeasureVAE / MeasureVAETrainer read from the reference's FolkNBarDataset"""
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


def test_decoder_accepts_multinomial_sampling():
    from arvae_amd.measure_vae import MeasureVAE
    torch.manual_seed(0)
    model = MeasureVAE(_FolkDataset(), 10, 2, 2, 64, 0.5, 16, 2, 64, 0.5, False, 'folk')
    dec = model.decoder
    assert dec.sampling == 'argmax' and dec.temperature == 1.0
    z, score = torch.zeros(3, 16), torch.zeros(3, 24, dtype=torch.int64)
    dec.use_teacher_forcing = False
    dec.sampling = 'multinomial'
    with pytest.raises(RuntimeError, match='no CPU fallback'):            # it is implemented: what is missing here is the GPU
        dec(z, score, True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec.generate(z)
    assert dec.sampling == 'multinomial' and dec.use_teacher_forcing is False and dec.temperature == 1.0     # generate restores
    dec.sampling = 'top_k'
    with pytest.raises(NotImplementedError):
        dec(z, score, True)
    with pytest.raises(NotImplementedError):
        dec.generate(z, sampling='nucleus')
    dec.sampling = 'multinomial'
    dec.temperature = 0.0
    with pytest.raises(ValueError, match='temperature'):
        dec(z, score, True)
    dec.temperature = 1.0
    dec.push_sampling_uniforms(torch.full((2, 24), 0.5))                    # a buffer of another batch size is refused
    with pytest.raises((ValueError, RuntimeError)):
        dec(z, score, True)
    with pytest.raises(AssertionError):
        model.forward_test(torch.zeros(3, 2, 23, dtype=torch.int64))

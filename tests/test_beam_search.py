"""Beam search of the MeasureVAE decoder, host side (include/arvae_hip.h, "Beam search"): the float64 restatement `beam64` of the
semantics and the follower `follow64` that tests/test_beam_search_gpu.py holds the device to, the share of ambiguous steps of the
float64 side alone on that file's cases, the three entry points' argument validation without a GPU, and the host-side checks of
beam_search / decode_latent_codes(sampling='beam') / the command line."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arvae_amd  # noqa: F401
from arvae_amd import _lib
from arvae_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_stack_ref as ref  # noqa: E402
from oracle.image_vae import selu  # noqa: E402
from oracle.measure_vae import BEATS, TICKS, TICKS_PER_BEAT  # noqa: E402
from test_sampling import _FolkDataset  # noqa: E402

DELTA = 1e-3                                                   # the clear margin (the filter tests' on weights)
# (B, hidden, vocab, layers, W) of tests/test_beam_search_gpu.py: each the smallest shape that reaches the path it names
CASES = [(21, 128, 35, 2, 4),      # ragged batch, three logits tiles
         (5, 32, 16, 2, 16),       # a code fills a 16-row tile, one logits tile
         (37, 64, 33, 2, 2),       # a tile boundary in the vocabulary
         (9, 64, 64, 2, 3),        # padded width, four tiles
         (301, 64, 35, 2, 4),      # more than 1024 rows: 8 rows per workgroup
         (600, 64, 35, 2, 4),      # 16 rows per workgroup
         (21, 64, 35, 1, 4),       # tick-by-tick path only
         (21, 64, 35, 3, 4)]       # tick-by-tick path only

# shapes no one-launch kernel is built for, beyond the layer counts above: another hidden size, more than 64 notes
OTHER_SHAPES = [(6, 48, 35, 2, 3), (6, 64, 70, 2, 3)]


def case_id(c):
    return f'b{c[0]}_h{c[1]}_v{c[2]}_l{c[3]}_w{c[4]}'


def make_decoder(hid, vocab, layers=2, seed=23):
    """test_sampling_filters_gpu._decoder on the CPU (the same parameters: they are drawn before any move to a device): output
    weights x 4, bias + 0.3, so that the notes vary and exact-zero logits stay off the cut"""
    from arvae_amd.measure_vae import HierarchicalDecoder
    torch.manual_seed(seed)
    dec = HierarchicalDecoder(10, vocab, 32, layers, hid, 0.0).train()
    with torch.no_grad():
        dec.tick_emb_to_note_emb[0].weight.mul_(4.0)
        dec.tick_emb_to_note_emb[0].bias.add_(0.3)
    dec.teacher_forcing_prob = 0.0
    return dec


def codes(b):
    return syn.normal_noise((b, 32), seed=29)


def half_mask(vocab):
    """a random half of the notes, note 0 banned"""
    allow = np.zeros(vocab, np.uint8)
    allow[np.random.RandomState(7).permutation(vocab)[:vocab // 2]] = 1
    allow[0] = 0
    return allow


def params64(dec):
    """the decoder's parameters as layer_stack_ref's float64 dict"""
    return {'decoder.' + k: v.detach().double().cpu() for k, v in dec.state_dict().items()}


# ---------------------------------------------------------------- the semantics, in float64
def logp64(logits, allow=None):
    """(..., V) float64 logits -> the log-softmax over the allowed notes, -inf at the banned ones"""
    l = np.asarray(logits, np.float64)
    a = np.ones(l.shape[-1], bool) if allow is None else np.asarray(allow).astype(bool)
    m = np.where(a, l, -np.inf).max(-1, keepdims=True)
    s = np.where(a, np.exp(l - m), 0.0).sum(-1, keepdims=True)
    return np.where(a, (l - m) - np.log(s), -np.inf)


def select64(scores, logp, width):
    """scores (B, K) (dead beams -inf), logp (B, K, V) -> (c (B, K*V) the candidates, order (B, K*V): c descending, ties to the lower
    k, then the lower v -- the flat index k*V + v ascending, a stable sort)"""
    with np.errstate(invalid='ignore'):
        c = scores[:, :, None] + logp
    c = np.where(np.isnan(c), -np.inf, c).reshape(c.shape[0], -1)
    return c, np.argsort(-c, axis=1, kind='stable')


class Stepper64:
    """the decoder's tick recurrence in float64 over (B, K) beams: step(t, parents, notes) -> logits (B, K, V) after feeding the
    chosen notes and taking the parents' states (None at tick 0)"""

    def __init__(self, p, z, width):
        self.p, self.k = p, width
        _, self.layers = ref.layer_counts(p)
        z = torch.as_tensor(np.asarray(z)).double()
        self.b = z.shape[0]
        hid = self.hid = p['decoder.rnn_beat.weight_hh_l0'].shape[1]
        split = lambda flat: [flat[:, i * hid:(i + 1) * hid] for i in range(self.layers)]
        h = split(selu(F.linear(z, p['decoder.z_to_beat_rnn_input.0.weight'], p['decoder.z_to_beat_rnn_input.0.bias'])))
        b0 = p['decoder.b_0'].reshape(1, 1).expand(self.b, 1)
        self.h0, self.bemb = [], []
        for i in range(BEATS):
            h = ref._stack_step(p, 'decoder.rnn_beat', self.layers, b0, h, None, i, 1.0)
            bo = h[-1]
            th = split(selu(F.linear(bo, p['decoder.beat_emb_to_tick_rnn_hidden.0.weight'], p['decoder.beat_emb_to_tick_rnn_hidden.0.bias'])))
            self.h0.append([s.repeat_interleave(width, 0) for s in th])
            self.bemb.append(selu(F.linear(bo, p['decoder.beat_emb_to_tick_rnn_input.0.weight'],
                                           p['decoder.beat_emb_to_tick_rnn_input.0.bias'])).repeat_interleave(width, 0))
        self.base = (torch.arange(self.b) * width)[:, None]
        self.prev = p['decoder.x_0'].reshape(1, -1).expand(self.b * width, -1)
        self.th = None

    def step(self, t, parents=None, notes=None):
        p = self.p
        if parents is not None:
            src = (self.base + torch.as_tensor(np.asarray(parents)).long()).reshape(-1)
            self.th = [s[src] for s in self.th]
            self.prev = p['decoder.note_embedding_layer.weight'][torch.as_tensor(np.asarray(notes)).long().reshape(-1)]
        i = t // TICKS_PER_BEAT
        if t % TICKS_PER_BEAT == 0:
            self.th = self.h0[i]                                           # every beam restarts from the beat's states
        self.th = ref._stack_step(p, 'decoder.rnn_tick', self.layers, torch.cat((self.prev, self.bemb[i]), 1), self.th, None, t, 1.0)
        probs = F.relu(F.linear(self.th[-1], p['decoder.tick_emb_to_note_emb.0.weight'], p['decoder.tick_emb_to_note_emb.0.bias']))
        return probs.numpy().reshape(self.b, self.k, -1)


class TableStepper:
    """hand-made logits: table[t][previous note] (V,) (row V: the start), the same for every code"""

    def __init__(self, table, b, width):
        self.table, self.b, self.k = np.asarray(table, np.float64), b, width
        self.v = self.table.shape[-1]

    def step(self, t, parents=None, notes=None):
        prev = np.full((self.b, self.k), self.v) if notes is None else np.asarray(notes)
        return self.table[t][prev]


def _gap(kth, nxt):
    """kth - nxt with inf where no further candidate exists (-inf on both sides included)"""
    with np.errstate(invalid='ignore'):
        g = kth - nxt
    return np.where(np.isnan(g), np.inf, g)


def backtrack(parents, tokens):
    """histories (B, T, W) -> the sequences (B, W, T), beam j of the last tick first"""
    b, ticks, w = tokens.shape
    at = np.broadcast_to(np.arange(w), (b, w)).copy()
    seq = np.zeros((b, w, ticks), np.int64)
    for t in range(ticks - 1, -1, -1):
        seq[:, :, t] = np.take_along_axis(tokens[:, t], at, 1)
        at = np.take_along_axis(parents[:, t].astype(np.int64), at, 1)
    return seq


def beam64(stepper, width, ticks=TICKS, allow=None):
    """-> dict(parents (B, T, W), tokens, scores (B, T, W), sequences (B, W, T), final (B, W), gap (B, T): c of the W-th minus c of the
    (W+1)-th candidate, inf when there is none)"""
    b = stepper.b
    scores = np.full((b, width), -np.inf)
    scores[:, 0] = 0.0                                                    # tick 0: one live beam
    out = dict(parents=[], tokens=[], scores=[], gap=[])
    par = note = None
    for t in range(ticks):
        logp = logp64(stepper.step(t, par, note), allow)
        v = logp.shape[-1]
        c, order = select64(scores, logp, width)
        top = order[:, :width]
        par, note = top // v, top % v
        scores = np.take_along_axis(c, top, 1)
        nxt = np.take_along_axis(c, order[:, width:width + 1], 1)[:, 0] if c.shape[1] > width else np.full(b, -np.inf)
        out['parents'].append(par), out['tokens'].append(note), out['scores'].append(scores), out['gap'].append(_gap(scores[:, -1], nxt))
    res = {k: np.stack(v, 1) for k, v in out.items()}
    res['sequences'], res['final'] = backtrack(res['parents'], res['tokens']), scores
    return res


def follow64(stepper, parents, tokens, width, allow=None):
    """carries float64 states and scores along a DEVICE history (parents, tokens (B, T, W)) -> dict over the ticks of, in float64:
    chosen (B, T, W) the candidate scores of the device's beams (= its beams' scores), kth (B, T) the W-th best candidate, gap (B, T)
    to the (W+1)-th, best_unchosen (B, T) the best candidate the device did not take, want_parents / want_tokens (B, T, W) float64's own
    first W.  A divergence at one tick never spoils the ticks after it: the next tick starts from the device's choice."""
    b, ticks, _ = tokens.shape
    scores = np.full((b, width), -np.inf)
    scores[:, 0] = 0.0
    out = dict(chosen=[], kth=[], gap=[], best_unchosen=[], want_parents=[], want_tokens=[])
    par = note = None
    for t in range(ticks):
        logp = logp64(stepper.step(t, par, note), allow)
        v = logp.shape[-1]
        c, order = select64(scores, logp, width)
        par, note = parents[:, t].astype(np.int64), tokens[:, t].astype(np.int64)
        flat = par * v + note
        chosen = np.take_along_axis(c, flat, 1)
        rest = c.copy()
        np.put_along_axis(rest, flat, -np.inf, 1)
        top = np.take_along_axis(c, order[:, :width + 1], 1)
        nxt = top[:, width] if top.shape[1] > width else np.full(b, -np.inf)
        out['chosen'].append(chosen), out['kth'].append(top[:, width - 1]), out['gap'].append(_gap(top[:, width - 1], nxt))
        out['best_unchosen'].append(rest.max(1))
        out['want_parents'].append(order[:, :width] // v), out['want_tokens'].append(order[:, :width] % v)
        scores = chosen
    return {k: np.stack(v, 1) for k, v in out.items()}


def check_history(fol, parents, tokens, width, delta=DELTA):
    """the device's selection against the follower, step by step -> (the ambiguous share, clear (B, T)): every chosen candidate has
    c64 >= T - delta, every candidate with c64 > T + delta is chosen, and at unambiguous steps (gap >= delta) the chosen
    (parent, note) list is float64's, in order"""
    kth = fol['kth'][..., None]
    assert np.isfinite(fol['chosen']).all()
    low = fol['chosen'] < kth - delta
    assert not low.any(), (np.argwhere(low)[:5], fol['chosen'][low][:5])
    missed = fol['best_unchosen'] > fol['kth'] + delta
    assert not missed.any(), np.argwhere(missed)[:5]
    clear = fol['gap'] >= delta
    np.testing.assert_array_equal(parents[clear], fol['want_parents'][clear])
    np.testing.assert_array_equal(tokens[clear], fol['want_tokens'][clear])
    return 1.0 - clear.mean(), clear


def test_float64_beam_restates_the_semantics():
    v = 5
    # tick 0 from the start row; afterwards rows by previous note.  Exact zero logits tie: decided by (k, v)
    zeros = np.zeros((3, v + 1, v))
    res = beam64(TableStepper(zeros, 2, 3), 3, ticks=3)
    np.testing.assert_array_equal(res['tokens'][0, 0], [0, 1, 2])        # one live beam: its first three notes
    np.testing.assert_array_equal(res['parents'][0, 0], [0, 0, 0])
    np.testing.assert_array_equal(res['tokens'][0, 1], [0, 1, 2])        # all 15 candidates tie: beam 0's first three notes
    np.testing.assert_array_equal(res['parents'][0, 1], [0, 0, 0])
    np.testing.assert_allclose(res['scores'][0, :, 0], -np.log(v) * np.arange(1, 4))
    assert (res['gap'] == 0).all()
    # distinct, sorted, and W = 1 is the argmax run (lowest index on ties)
    rs = np.random.RandomState(3)
    table = np.maximum(rs.normal(size=(6, v + 1, v)) * 2.0, 0.0)
    table[2, :, :] = 0.0                                                  # a tick of ties
    res = beam64(TableStepper(table, 1, 4), 4, ticks=6)
    seqs = [tuple(s) for s in res['sequences'][0]]
    assert len(set(seqs)) == 4 and (np.diff(res['final'][0]) <= 0).all() and np.isfinite(res['final']).all()
    # the score of a sequence is the sum of its notes' log-softmax
    for s, f in zip(seqs, res['final'][0]):
        prev, total = v, 0.0
        for t, n in enumerate(s):
            total += logp64(table[t][prev])[n]
            prev = n
        assert abs(total - f) < 1e-12
    # exhaustive: with W = 25 no two-tick prefix is dropped, so the first beam is the best of all 5^3 three-tick measures
    full = beam64(TableStepper(table, 1, 25), 25, ticks=3)
    best, arg = -np.inf, None
    for a in range(v):
        for b_ in range(v):
            for c in range(v):
                s = logp64(table[0][v])[a] + logp64(table[1][a])[b_] + logp64(table[2][b_])[c]
                if s > best + 1e-15:
                    best, arg = s, (a, b_, c)
    assert tuple(full['sequences'][0, 0]) == arg and abs(full['final'][0, 0] - best) < 1e-12
    greedy = beam64(TableStepper(table, 1, 1), 1, ticks=6)
    prev = v
    for t in range(6):
        assert greedy['tokens'][0, t, 0] == int(np.argmax(table[t][prev]))
        prev = int(np.argmax(table[t][prev]))
    # a mask: the softmax is over the allowed notes only, banned notes never appear; a mask of W notes at tick 0 gives exactly those
    allow = np.array([0, 1, 0, 1, 1], np.uint8)
    res = beam64(TableStepper(table, 1, 3), 3, ticks=6, allow=allow)
    assert allow[res['tokens']].all() and sorted(res['tokens'][0, 0]) == [1, 3, 4]
    lp = logp64(table[0][v], allow)
    np.testing.assert_array_equal(res['tokens'][0, 0], np.argsort(-lp, kind='stable')[:3])
    assert abs(np.exp(lp[allow.astype(bool)]).sum() - 1.0) < 1e-12
    # the follower on beam64's own history: every step agrees, nothing is ambiguous beyond the ties
    fol = follow64(TableStepper(table, 1, 4), *[beam64(TableStepper(table, 1, 4), 4, ticks=6)[k] for k in ('parents', 'tokens')], 4)
    ref4 = beam64(TableStepper(table, 1, 4), 4, ticks=6)
    np.testing.assert_allclose(fol['chosen'], ref4['scores'], atol=1e-12)
    np.testing.assert_array_equal(fol['want_tokens'], ref4['tokens'])
    np.testing.assert_array_equal(backtrack(ref4['parents'], ref4['tokens']), ref4['sequences'])


def test_float64_decoder_beam_of_width_one_is_the_argmax_run():
    dec = make_decoder(64, 35, 3)
    p = params64(dec)
    z = codes(6)
    res = beam64(Stepper64(p, z, 1), 1)
    _, samples = ref.decode(p, torch.from_numpy(z).double(), None, False)
    np.testing.assert_array_equal(res['sequences'][:, 0], samples[:, 0].numpy())
    wide = beam64(Stepper64(p, z, 4), 4)
    for b in range(6):
        assert len({tuple(s) for s in wide['sequences'][b]}) == 4
    assert (np.diff(wide['final'], axis=1) <= 0).all()


AMBIGUOUS = {}


def ambiguous_share(case, masked):
    """the float64 reference's own share of steps whose W-th and (W+1)-th candidates lie within DELTA"""
    if (case, masked) not in AMBIGUOUS:
        b, hid, vocab, layers, w = case
        p = params64(make_decoder(hid, vocab, layers))
        res = beam64(Stepper64(p, codes(b), w), w, allow=half_mask(vocab) if masked else None)
        AMBIGUOUS[(case, masked)] = float((res['gap'] < DELTA).mean())
    return AMBIGUOUS[(case, masked)]


@pytest.mark.parametrize('case', CASES + OTHER_SHAPES, ids=[case_id(c) for c in CASES + OTHER_SHAPES])
def test_float64_reference_is_rarely_ambiguous_on_the_device_cases(case):
    """the cap the device tests assert (5 %) is met by the float64 side alone, with and without the half mask: beyond it a device test
    would prove nothing"""
    for masked in (False, True):
        if masked and case[4] > case[2] // 2 - 1:
            continue                                                      # (the half mask leaves fewer notes than the width)
        share = ambiguous_share(case, masked)
        print(f'beam case {case_id(case)} mask {masked}: float64 ambiguous steps {share:.4f}')
        assert share <= 0.05


# ---------------------------------------------------------------- the library's entry points without a GPU
@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _err(lib):
    return lib.arvae_last_error_string().decode()


P = ctypes.c_void_p(256)                                       # never dereferenced: every call below fails validation first


def test_beam_select_rejects_bad_arguments(lib):
    def call(logits=P, scores=P, codes=2, width=4, vocab=35, live=4, allow=None, allowed=35, parents=P, notes=P, out=P):
        return lib.arvae_beam_select(logits, scores, codes, width, vocab, live, allow, allowed, parents, notes, out, None)
    for kw in ({'logits': None}, {'scores': None}, {'parents': None}, {'notes': None}, {'out': None}):
        assert call(**kw) == -1 and 'beam_select' in _err(lib) and 'null pointer' in _err(lib), kw
    for width in (0, -1, 17):
        assert call(width=width, live=1) == -1 and 'width' in _err(lib) and '[1, 16]' in _err(lib)
    assert call(codes=0) == -1 and 'codes' in _err(lib)
    assert call(vocab=0) == -1 and 'vocab' in _err(lib)
    assert call(allow=P, allowed=3) == -1 and 'width 4 is above the 3 allowed notes' in _err(lib)
    assert call(vocab=3, allowed=3) == -1 and 'above the 3 allowed' in _err(lib)
    assert call(allowed=20) == -1 and 'allowed' in _err(lib) and 'without a mask' in _err(lib)
    assert call(allow=P, allowed=36) == -1 and call(allow=P, allowed=0) == -1 and 'allowed' in _err(lib)
    for live in (0, 5, -2):
        assert call(live=live) == -1 and 'live' in _err(lib)
    assert call(width=8, vocab=4, allowed=4, live=1) == -1 and 'width' in _err(lib)


def test_sequence_log_prob_rejects_bad_arguments(lib):
    def call(w=P, tok=P, rows=3, steps=24, vocab=35, allow=None, out=P):
        return lib.arvae_sequence_log_prob(w, tok, rows, steps, vocab, allow, out, None)
    for kw in ({'w': None}, {'tok': None}, {'out': None}):
        assert call(**kw) == -1 and 'sequence_log_prob' in _err(lib) and 'null pointer' in _err(lib), kw
    for name in ('rows', 'steps', 'vocab'):
        assert call(**{name: 0}) == -1 and name in _err(lib)


def test_tick_beam_search_rejects_bad_arguments(lib):
    tw = _lib.TickWeights(*([P] * 8))
    aligned, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)

    def call(weights=tw, h0=P, h1=P, stride=0, gib=P, ptab=P, batch=3, beats=4, tpb=6, hidden=64, vocab=35, width=4, allow=None,
             allowed=35, parents=P, tokens=P, hist=P, seqs=P, scores=P, ws=aligned):
        return lib.arvae_tick_beam_search(ctypes.byref(weights) if weights is not None else None, h0, h1, stride, gib, ptab, batch, beats, tpb,
                                          hidden, vocab, width, allow, allowed, parents, tokens, hist, seqs, scores, ws, None)
    for kw in ({'weights': None}, {'h0': None}, {'h1': None}, {'gib': None}, {'ptab': None}):
        assert call(**kw) == -1 and 'tick_beam_search' in _err(lib) and 'null pointer' in _err(lib), kw
    holes = _lib.TickWeights(*([P] * 7 + [None]))
    assert call(weights=holes) == -1 and 'null weight pointer' in _err(lib)
    for kw in ({'parents': None}, {'tokens': None}, {'hist': None}, {'seqs': None}, {'scores': None}):
        assert call(**kw) == -1 and 'null output pointer' in _err(lib), kw
    assert call(ws=None) == -1 and 'workspace' in _err(lib)
    assert call(ws=odd) == -1 and 'workspace' in _err(lib) and 'aligned' in _err(lib)
    for width in (0, 17, -3):
        assert call(width=width) == -1 and 'width' in _err(lib) and '[1, 16]' in _err(lib)
    assert call(allow=P, allowed=3) == -1 and 'width 4 is above the 3 allowed notes' in _err(lib)
    assert call(allowed=12) == -1 and 'without a mask' in _err(lib)
    assert call(hidden=48) == -1 and 'hidden size 48' in _err(lib)
    assert call(vocab=65, allowed=65) == -1 and 'vocab' in _err(lib)
    assert call(hidden=32, vocab=35) == -1 and 'vocab' in _err(lib)      # more notes than a hidden-32 workgroup has logits lanes
    assert call(batch=0) == -1 and call(beats=0) == -1 and 'empty problem' in _err(lib)
    assert call(beats=6) == -1 and 'ticks' in _err(lib)                  # 36 ticks: above what the kernel keeps
    assert call(stride=8) == -1 and 'h0_stride' in _err(lib)
    assert lib.arvae_tick_beam_search_supported(128, 35, 4) == 1 and lib.arvae_tick_beam_search_supported(64, 64, 16) == 1
    assert lib.arvae_tick_beam_search_supported(128, 35, 17) == 0 and lib.arvae_tick_beam_search_supported(128, 35, 0) == 0
    assert lib.arvae_tick_beam_search_supported(96, 35, 4) == 0 and lib.arvae_tick_beam_search_supported(64, 65, 4) == 0
    assert lib.arvae_tick_beam_search_ws_floats(128) == lib.arvae_tick_free_run_ws_floats(128) > 0
    assert lib.arvae_tick_beam_search_ws_floats(48) == 0


NAMES = ('arvae_beam_select', 'arvae_sequence_log_prob', 'arvae_tick_beam_search_supported', 'arvae_tick_beam_search_ws_floats',
         'arvae_tick_beam_search')


def test_new_entry_points_are_bound_and_declared_once(lib):
    header = open(os.path.join(ROOT, 'include', 'arvae_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(re.findall(r'^int(?:64_t)? ' + name + r'\(', header, re.M)) == 1, name
    assert lib.arvae_abi_version() == 16 == _lib.ABI_VERSION
    assert re.search(r'#define ARVAE_ABI_VERSION\s+16\b', header)


# ---------------------------------------------------------------- the host side of beam_search / decode_latent_codes / the CLI
def _model_and_trainer():
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    torch.manual_seed(0)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.5, 16, 2, 64, 0.5, False, 'folk')
    return ds, model, MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))


def test_beam_search_validates_its_arguments_on_the_host():
    ds, model, trainer = _model_and_trainer()
    dec = model.decoder
    dec.train()
    z = torch.zeros(3, 16)
    three = np.zeros(35, np.uint8)
    three[[4, 9, 20]] = 1
    for kw in ({'beam_width': 0}, {'beam_width': 17}, {'beam_width': -1}, {'beam_width': 4, 'allowed': three},
               {'allowed': np.zeros(35, np.uint8)}, {'allowed': np.ones(34, np.uint8)}, {'allowed': np.full(35, 2, np.uint8)}):
        with pytest.raises(ValueError):
            dec.beam_search(z, **kw)
    for kw in ({'beam_width': 2.5}, {'beam_width': True}, {'beam_width': '4'}, {'allowed': np.ones(35, np.float32)}):
        with pytest.raises(TypeError):
            dec.beam_search(z, **kw)
    with pytest.raises(ValueError, match='above the 3 allowed'):
        dec.beam_search(z, beam_width=4, allowed=three)
    # valid arguments get as far as the device: what is missing here is the GPU, and the decoder is left as it was
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec.beam_search(z, beam_width=3, allowed=three)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec.score_tokens(z, torch.zeros(3, 24, dtype=torch.int64))
    assert dec.training and dec.use_teacher_forcing is True and dec.sampling == 'argmax' and dec._filter is None
    # the trainer: 'beam' draws nothing
    codes_ = torch.zeros(2, 16)
    for kw in ({'top_k': 3}, {'top_p': 0.9}, {'temperature': 0.8}, {'uniforms': torch.ones(2, 24)}):
        with pytest.raises(ValueError, match='beam'):
            trainer.decode_latent_codes(codes_, sampling='beam', **kw)
    with pytest.raises(ValueError):
        trainer.decode_latent_codes(codes_, sampling='beam', beam_width=17)
    pads = np.zeros(35, np.uint8)
    pads[[ds.note2index_dicts['START'], ds.note2index_dicts['END'], 20]] = 1
    with pytest.raises(ValueError, match='above the 1 allowed'):          # once the padding symbols go, one note is left
        trainer.decode_latent_codes(codes_, sampling='beam', beam_width=2, allowed=pads, playable=True)
    with pytest.raises(ValueError):
        trainer.sample_measures(4, beam_width=4, top_k=3)
    with pytest.raises(ValueError):
        trainer.sample_measures(4, beam_width=0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        trainer.decode_latent_codes(codes_, sampling='beam', beam_width=4, playable=True)


def test_cli_rejects_beam_with_the_draws_flags():
    sys.path.insert(0, ROOT)
    import train_measure_vae as cli
    for args in (['--sample', '2', '--beam', '4', '--top_k', '3'], ['--sample', '2', '--beam', '4', '--top_p', '0.9'],
                 ['--sample', '2', '--beam=4', '--temperature', '0.8'], ['--sample', '2', '--beam', '4', '--temperature=1.0'],
                 ['--sample', '2', '--beam', '0'], ['--sample', '2', '--beam', '17']):
        with pytest.raises(ValueError, match='--beam'):
            cli.run(args)
    assert '--beam' in cli.SAMPLE_HELP

"""Note plans of the MeasureVAE decoder (include/arvae_hip.h, arvae_note_plan_t), host side: the float64 restatement of the
semantics -- the filtered draw with a per-(row, tick) allowed set, the beam search whose banned candidates are excluded and whose
slots without a candidate are dead -- and the follower tests/test_note_plan_gpu.py holds the device to, the ambiguous share of the
float64 side alone on that file's cases, the six new entry points' argument validation and the struct's layout without a GPU, and the
host-side checks of note_plan / build_note_plan / infill_measures / the command line."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import arvae_amd  # noqa: F401
from arvae_amd import _lib
from oracle import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_beam_search import (DELTA, Stepper64, TableStepper, _gap, backtrack, codes, logp64, make_decoder, params64,  # noqa: E402
                              select64)
from test_sampling_filters import _model_and_trainer, check_tick_picks, filter64, pick64_filtered  # noqa: E402

TICKS = 24
CAP64 = 0.03                                                   # the float64 side alone; the device tests assert 0.05
# (B, hidden, vocab, layers, top_k, top_p, tau): the filtered draws under the plan
PICK_CASES = [(21, 128, 35, 2, 4, 0.8, 0.6), (37, 64, 16, 2, 3, 0.7, 0.5), (45, 32, 32, 2, 5, 0.8, 0.7), (64, 128, 64, 2, 3, 0.6, 0.5),
              (21, 64, 35, 1, 3, 0.7, 0.5), (21, 64, 35, 3, 4, 0.8, 0.6)]
# always tick by tick: hidden 128 with three layers, vocabulary 35 at hidden 32
PICK_STEPWISE_ONLY = [(21, 128, 35, 3, 4, 0.8, 0.6), (21, 32, 35, 2, 5, 0.8, 0.7)]
# (B, hidden, vocab, layers, W): the beam searches under the plan
BEAM_CASES = [(21, 128, 35, 2, 4), (5, 32, 16, 2, 16), (37, 64, 33, 2, 2), (9, 64, 64, 2, 3), (21, 64, 35, 1, 4), (21, 64, 35, 3, 4)]


def pick_id(c):
    return f'b{c[0]}_h{c[1]}_v{c[2]}_l{c[3]}_k{c[4]}_p{c[5]}_t{c[6]}'


def beam_id(c):
    return f'b{c[0]}_h{c[1]}_v{c[2]}_l{c[3]}_w{c[4]}'


# ---------------------------------------------------------------- the plan of every test, the draws
FREE, FORCED, SUBSET = 0, 1, 2


def make_plan(b, vocab, seed=101):
    """uint8 (b, 24, vocab): per (row, tick) a kind drawn uniformly from three -- free: everything but note 0; forced: one random
    note; subset: a random max(2, V // 2) notes.  Row 0 is forced at all 24 ticks, row 1 free at all, row 2 subset at all.  One
    RandomState(seed): the kinds first, then per (row, tick) in order what its kind needs."""
    rs = np.random.RandomState(seed)
    kinds = rs.randint(0, 3, size=(b, TICKS))
    for row, kind in ((0, FORCED), (1, FREE), (2, SUBSET)):
        if row < b:
            kinds[row] = kind
    plan = np.zeros((b, TICKS, vocab), np.uint8)
    for row in range(b):
        for t in range(TICKS):
            if kinds[row, t] == FREE:
                plan[row, t, 1:] = 1
                if vocab == 1:
                    plan[row, t, 0] = 1
            elif kinds[row, t] == FORCED:
                plan[row, t, rs.randint(vocab)] = 1
            else:
                plan[row, t, rs.permutation(vocab)[:max(2, vocab // 2)]] = 1
    return plan


def draws(b, edges=False):
    """(b, 24) float32 in (0, 1], those of test_sampling_filters_gpu._inputs: edges = every third row draws u = 1 at every tick
    and row 1 the smallest u, 2^-32"""
    u = np.asarray(philox.unit(philox.blocks(b * TICKS, 1234, 7, 0)[:, 0]), np.float32).reshape(b, TICKS)
    if edges:
        u[::3] = 1.0
        u[1] = 2.0 ** -32
    return u


def allowed_counts(plan):
    """|A(b, t)| (B, T) as Python-int-safe int64"""
    return (np.asarray(plan) != 0).sum(-1).astype(np.int64)


def finite_counts(plan, width):
    """(B, T): how many hypotheses of a code are finite after tick t = min(W, prod over s <= t of |A(b, s)|), in integer arithmetic"""
    n = allowed_counts(plan)
    out = np.zeros(n.shape, np.int64)
    for row in range(n.shape[0]):
        prod = 1
        for t in range(n.shape[1]):
            prod = min(width, prod * int(n[row, t]))
            out[row, t] = prod
    return out


# ---------------------------------------------------------------- the planned beam search, in float64
def plan_logp64(logits, allow):
    """(B, K, V) logits, allow (B, V) -> the log-softmax over each code's allowed notes, -inf at the others"""
    l = np.asarray(logits, np.float64)
    a = np.asarray(allow).astype(bool)[:, None, :]
    m = np.where(a, l, -np.inf).max(-1, keepdims=True)
    s = np.where(a, np.exp(l - m), 0.0).sum(-1, keepdims=True)
    return np.where(a, (l - m) - np.log(s), -np.inf)


def _candidates(scores, logits, allow, width):
    """-> (c (B, K*V) with -inf where there is NO candidate, order, ncand (B,)): the candidates of a code are (k, v) with beam k finite
    and v allowed -- the others are excluded: they are not candidates of score -inf.  (A finite beam and an allowed note always give a
    finite c, so the -inf entries of c are exactly the excluded ones.)"""
    live = np.isfinite(scores)
    a = np.asarray(allow).astype(bool)
    c, order = select64(np.where(live, scores, -np.inf), plan_logp64(logits, a), width)
    ncand = live.sum(1) * a.sum(1)
    assert (np.isfinite(c).sum(1) == ncand).all()
    return c, order, ncand


def beam64_plan(stepper, width, plan, ticks=TICKS):
    """the planned search -> dict(parents, tokens, scores (B, T, W), finite (B, T, W) bool, sequences (B, W, T), final (B, W), gap (B, T):
    c of the last finite pick minus c of the best candidate left, inf when none is left).  Dead slots: score -inf, parent 0, the
    code's first allowed note."""
    b = stepper.b
    scores = np.full((b, width), -np.inf)
    scores[:, 0] = 0.0
    out = dict(parents=[], tokens=[], scores=[], gap=[])
    par = note = None
    for t in range(ticks):
        allow = np.asarray(plan)[:, t] != 0
        logits = stepper.step(t, par, note)
        v = logits.shape[-1]
        c, order, ncand = _candidates(scores, logits, allow, width)
        top = order[:, :width]
        scores = np.take_along_axis(c, top, 1)                            # (-inf beyond the candidates: the dead slots)
        dead = ~np.isfinite(scores)
        par = np.where(dead, 0, top // v)
        note = np.where(dead, allow.argmax(1)[:, None], top % v)
        nfin = np.minimum(width, ncand)
        last = np.take_along_axis(scores, (nfin - 1)[:, None], 1)[:, 0]
        nxt = np.take_along_axis(c, order[:, width:width + 1], 1)[:, 0] if c.shape[1] > width else np.full(b, -np.inf)
        nxt = np.where(ncand > width, nxt, -np.inf)
        out['parents'].append(par), out['tokens'].append(note), out['scores'].append(scores), out['gap'].append(_gap(last, nxt))
    res = {k: np.stack(v, 1) for k, v in out.items()}
    res['finite'] = np.isfinite(res['scores'])
    res['sequences'], res['final'] = backtrack(res['parents'], res['tokens']), scores
    return res


def follow64_plan(stepper, parents, tokens, finite, width, plan):
    """carries float64 states and scores along a DEVICE history (parents, tokens (B, T, W); finite (B, T, W): the slots whose device
    score is finite) -> dict over the ticks of, in float64: nfin (B, T) = min(W, candidates), chosen (B, T, W) the candidate scores of
    the device's finite slots (-inf: a dead slot, or a finite slot that is no candidate at all), kth (B, T) the nfin-th best
    candidate, gap (B, T) to the next one, best_unchosen (B, T), want_parents / want_tokens (B, T, W) float64's own first W.  The
    next tick starts from the device's choice."""
    b, ticks, _ = tokens.shape
    scores = np.full((b, width), -np.inf)
    scores[:, 0] = 0.0
    out = dict(nfin=[], chosen=[], kth=[], gap=[], best_unchosen=[], want_parents=[], want_tokens=[])
    par = note = None
    for t in range(ticks):
        allow = np.asarray(plan)[:, t] != 0
        logits = stepper.step(t, par, note)
        v = logits.shape[-1]
        c, order, ncand = _candidates(scores, logits, allow, width)
        nfin = np.minimum(width, ncand)
        par, note = parents[:, t].astype(np.int64), tokens[:, t].astype(np.int64)
        flat = par * v + note
        chosen = np.where(finite[:, t], np.take_along_axis(c, flat, 1), -np.inf)
        rest = c.copy()
        for j in range(width):                                            # (only the finite slots take a candidate away)
            rows = np.flatnonzero(finite[:, t, j])
            rest[rows, flat[rows, j]] = -np.inf
        top = np.take_along_axis(c, order[:, :width + 1], 1)
        kth = np.take_along_axis(top, (nfin - 1)[:, None], 1)[:, 0]
        nxt = np.where(ncand > nfin, np.take_along_axis(top, np.minimum(nfin, top.shape[1] - 1)[:, None], 1)[:, 0], -np.inf)
        out['nfin'].append(nfin), out['chosen'].append(chosen), out['kth'].append(kth), out['gap'].append(_gap(kth, nxt))
        out['best_unchosen'].append(rest.max(1))
        out['want_parents'].append(order[:, :width] // v), out['want_tokens'].append(order[:, :width] % v)
        scores = chosen
    return {k: np.stack(v, 1) for k, v in out.items()}


def check_history_plan(fol, parents, tokens, hist, plan, width, delta=DELTA):
    """the device's planned selection against the follower -> (the ambiguous share, clear (B, T)).  The number of finite slots is
    min(W, candidates) and min(W, prod |A|), exactly; they are listed first, in non-increasing order; every finite chosen candidate
    has c64 >= kth - delta, no candidate with c64 > kth + delta is left out, and at clear steps (gap >= delta) the finite
    (parent, note) list is float64's, in order.  Dead slots score -inf, and EVERY token, dead or not, is inside its tick's A(b, t)."""
    finite = np.isfinite(hist)
    assert not np.isnan(hist).any() and (hist[~finite] == -np.inf).all()
    np.testing.assert_array_equal(finite.sum(-1), fol['nfin'])
    np.testing.assert_array_equal(fol['nfin'], finite_counts(plan, width))
    assert (np.diff(finite.astype(np.int8), axis=-1) <= 0).all()          # dead slots last
    with np.errstate(invalid='ignore'):
        assert not (np.diff(hist, axis=-1) > 0).any()                     # best first
    b, ticks, _ = tokens.shape
    rows, ts = np.arange(b)[:, None, None], np.arange(ticks)[None, :, None]
    assert tokens.min() >= 0 and tokens.max() < plan.shape[-1] and parents.min() >= 0 and parents.max() < width
    assert (np.asarray(plan)[rows, ts, tokens] != 0).all()
    kth = fol['kth'][..., None]
    low = finite & (fol['chosen'] < kth - delta)
    assert not low.any(), (np.argwhere(low)[:5], fol['chosen'][low][:5])
    missed = fol['best_unchosen'] > fol['kth'] + delta
    assert not missed.any(), np.argwhere(missed)[:5]
    clear = fol['gap'] >= delta
    sel = clear[..., None] & finite
    np.testing.assert_array_equal(parents[sel], fol['want_parents'][sel])
    np.testing.assert_array_equal(tokens[sel], fol['want_tokens'][sel])
    return 1.0 - clear.mean(), clear


# ---------------------------------------------------------------- 1. the semantics on hand-made logits
def test_float64_planned_picks_restate_the_semantics():
    l = np.array([0.0, 3.0, 0.0, 1.0, 0.0, 2.0])
    # a forced tick: the one allowed note at every draw, whatever the cuts
    for note in range(6):
        one = np.zeros(6, np.uint8)
        one[note] = 1
        for u in (2.0 ** -32, 0.4, 1.0):
            for kw in ({}, {'top_k': 1}, {'top_k': 3, 'top_p': 0.2}):
                assert pick64_filtered(l, u, 0.7, allow=one, **kw)[0] == note
    # the ranks, the maximum and S are taken among A(b, t): with note 1 (the largest) banned, top_k = 2 keeps 5 and 3, and
    # note 3's mass_before is e_5 / (e_5 + e_3) = 1 / (1 + e^-1) = 0.731 -- not e_5 / (the sum with note 1)
    a = np.array([1, 0, 1, 1, 1, 1], np.uint8)
    np.testing.assert_array_equal(np.flatnonzero(filter64(l, a, 2, 1.0, 1.0)), [3, 5])
    assert filter64(l, a, 2, 0.72, 1.0).sum() == 1 and filter64(l, a, 2, 0.74, 1.0).sum() == 2
    # a (B, 24, V) plan broadcasts: every (row, tick) has its own set
    plan = make_plan(4, 6)
    logits = np.maximum(np.random.RandomState(5).normal(size=(4, TICKS, 6)) * 2.0, 0.0)
    u = draws(4, edges=True)
    tok = pick64_filtered(logits, u, 0.8, plan, 3, 0.9)[0]
    assert np.take_along_axis(plan, tok[..., None], -1).all()
    np.testing.assert_array_equal(tok[0], plan[0].argmax(-1))              # row 0 is forced throughout
    assert (plan[1] == np.array([0, 1, 1, 1, 1, 1])).all() and (plan[2].sum(-1) == 3).all()
    # argmax under a plan is the top_k = 1 rule: the allowed note with the largest logit, ties to the lower index, at every draw
    want = np.where(plan != 0, logits, -1.0).argmax(-1)
    for uu in (u, np.ones_like(u), np.full_like(u, 2.0 ** -32)):
        np.testing.assert_array_equal(pick64_filtered(logits, uu, 0.8, plan, 1, 1.0)[0], want)
    ties = np.zeros((1, 1, 6))
    assert pick64_filtered(ties, np.ones((1, 1)), 1.0, np.array([[[0, 0, 1, 0, 1, 1]]]), 1, 1.0)[0][0, 0] == 2


def test_float64_planned_beam_restates_the_semantics():
    v, w, ticks = 5, 4, 6
    rs = np.random.RandomState(3)
    table = np.maximum(rs.normal(size=(ticks, v + 1, v)) * 2.0, 0.05) + rs.random_sample((ticks, v + 1, v)) * 1e-3     # distinct scores
    # a forced first tick leaves one finite hypothesis and W - 1 dead slots; the forced tick adds exactly 0.0
    plan = np.ones((1, ticks, v), np.uint8)
    plan[0, 0] = [0, 0, 1, 0, 0]
    res = beam64_plan(TableStepper(table, 1, w), w, plan, ticks)
    assert res['finite'][0, 0].tolist() == [True, False, False, False] and res['scores'][0, 0, 0] == 0.0
    assert res['tokens'][0, 0].tolist() == [2, 2, 2, 2] and (res['scores'][0, 0, 1:] == -np.inf).all()
    assert res['finite'][0, 1].all()                                     # 5 candidates at the next tick: all four slots finite
    # the finite count is min(W, prod |A|), every sequence obeys the plan, dead slots stay dead and come last
    plan = np.ones((3, ticks, v), np.uint8)
    plan[0, :, :] = 0
    plan[0, np.arange(ticks), rs.randint(0, v, ticks)] = 1                 # forced throughout: one hypothesis
    plan[1, :3, :] = [0, 1, 0, 0, 0]
    plan[1, 3] = [1, 0, 0, 1, 0]                                           # 1, 1, 1, 2, then 5: two, then four
    plan[2, 0] = [1, 1, 0, 0, 0]
    plan[2, 1:] = [0, 0, 0, 0, 1]                                          # two hypotheses for good
    res = beam64_plan(TableStepper(table, 3, w), w, plan, ticks)
    np.testing.assert_array_equal(res['finite'].sum(-1), finite_counts(plan, w))
    assert finite_counts(plan, w)[:, -1].tolist() == [1, 4, 2]
    assert (np.diff(res['finite'].astype(int), axis=-1) <= 0).all()
    rows, ts = np.arange(3)[:, None, None], np.arange(ticks)[None, :, None]
    assert (plan[rows, ts, res['tokens']] != 0).all()
    assert (plan[np.arange(3)[:, None, None], np.arange(ticks)[None, None, :], res['sequences']] != 0).all()
    np.testing.assert_array_equal(res['sequences'][0, 0], plan[0].argmax(-1))
    assert res['final'][0, 0] == 0.0                                      # 24 forced ticks add exactly nothing
    fin = res['finite'][:, -1]
    with np.errstate(invalid='ignore'):
        assert not (np.diff(np.where(fin, res['final'], -np.inf), axis=1) > 0).any()
    for code in range(3):
        seqs = {tuple(s) for s, f in zip(res['sequences'][code], fin[code]) if f}
        assert len(seqs) == fin[code].sum()                               # the finite hypotheses are distinct
    # the score of a finite sequence is the sum over ticks of the log-softmax over A(b, t)
    for code in range(3):
        for s, f, score in zip(res['sequences'][code], fin[code], res['final'][code]):
            if not f:
                continue
            prev, total = v, 0.0
            for t, n in enumerate(s):
                total += logp64(table[t][prev], plan[code, t])[n]
                prev = n
            assert abs(total - score) < 1e-12
    # a plan of all ones is the search without a plan; a plan that repeats one mask is the search with allow = that mask
    from test_beam_search import beam64
    for allow in (None, np.array([0, 1, 0, 1, 1], np.uint8)):
        rep = np.broadcast_to(np.ones(v, np.uint8) if allow is None else allow, (2, ticks, v))
        got, want = beam64_plan(TableStepper(table, 2, 3), 3, rep, ticks), beam64(TableStepper(table, 2, 3), 3, ticks=ticks, allow=allow)
        for key in ('parents', 'tokens', 'scores', 'sequences', 'final'):
            np.testing.assert_array_equal(got[key], want[key])
    # the follower on the search's own history agrees with it at every step
    fol = follow64_plan(TableStepper(table, 3, w), res['parents'], res['tokens'], res['finite'], w, plan)
    np.testing.assert_array_equal(fol['chosen'], res['scores'])
    share, clear = check_history_plan(fol, res['parents'], res['tokens'], res['scores'], plan, w)
    assert clear.shape == (3, ticks)


# ---------------------------------------------------------------- 2. the float64 side alone on the device tests' cases
_PICKS64, _BEAMS64 = {}, {}


def picks64(case):
    """the float64 decoder's free run under the plan (Stepper64 at width 1, the emitted note fed back) -> (tokens, weights (B, 24, V),
    u, plan)"""
    if case not in _PICKS64:
        b, hid, vocab, layers, top_k, top_p, tau = case
        step = Stepper64(params64(make_decoder(hid, vocab, layers)), codes(b), 1)
        plan, u = make_plan(b, vocab), draws(b)
        out = {}
        for name, (k, p) in (('draw', (top_k, top_p)), ('argmax', (1, 1.0))):
            step.prev, step.th = step.p['decoder.x_0'].reshape(1, -1).expand(b, -1), None
            toks, ws, note = [], [], None
            for t in range(TICKS):
                w = step.step(t, None if note is None else np.zeros((b, 1), np.int64), note)[:, 0]
                tok = pick64_filtered(w, u[:, t], tau, plan[:, t], k, p)[0]
                toks.append(tok), ws.append(w)
                note = tok[:, None]
            out[name] = (np.stack(toks, 1), np.stack(ws, 1))
        _PICKS64[case] = (out, u, plan)
    return _PICKS64[case]


@pytest.mark.parametrize('case', PICK_CASES + PICK_STEPWISE_ONLY, ids=[pick_id(c) for c in PICK_CASES + PICK_STEPWISE_ONLY])
def test_float64_planned_draws_are_rarely_ambiguous(case):
    """what tests/test_note_plan_gpu.py caps at 0.05 on the device is met by the float64 side alone (0.03), for the planned draws
    and the planned argmax: beyond it a device test would prove nothing.  Bands: eps = 1e-5 max|w| + 1e-6, delta = 2 eps / tau + 1e-5."""
    b, hid, vocab, layers, top_k, top_p, tau = case
    out, u, plan = picks64(case)
    for name, (k, p) in (('draw', (top_k, top_p)), ('argmax', (1, 1.0))):
        tok, w = out[name]
        assert np.take_along_axis(plan, tok[..., None], -1).all()
        np.testing.assert_array_equal(tok[0], plan[0].argmax(-1))
        eps = 1e-5 * float(np.abs(w).max()) + 1e-6
        delta = 2.0 * eps / tau + 1e-5
        share, _ = check_tick_picks(tok, w, u, tau, plan, k, p, eps, delta)
        print(f'planned {name} case {pick_id(case)}: float64 ambiguous draws {share:.4f}')
        assert share <= CAP64
        assert len(np.unique(tok)) > 3


def beams64(case):
    if case not in _BEAMS64:
        b, hid, vocab, layers, w = case
        _BEAMS64[case] = beam64_plan(Stepper64(params64(make_decoder(hid, vocab, layers)), codes(b), w), w, make_plan(b, vocab))
    return _BEAMS64[case]


@pytest.mark.parametrize('case', BEAM_CASES, ids=[beam_id(c) for c in BEAM_CASES])
def test_float64_planned_beams_are_rarely_ambiguous(case):
    b, hid, vocab, layers, w = case
    res, plan = beams64(case), make_plan(b, vocab)
    share = float((res['gap'] < DELTA).mean())
    print(f'planned beam case {beam_id(case)}: float64 ambiguous steps {share:.4f}')
    assert share <= CAP64
    np.testing.assert_array_equal(res['finite'].sum(-1), finite_counts(plan, w))
    assert res['finite'][0, -1].sum() == 1 and res['finite'][1, -1].sum() == w      # row 0 forced: one hypothesis; row 1 free: W
    np.testing.assert_array_equal(res['sequences'][0, 0], plan[0].argmax(-1))
    assert res['final'][0, 0] == 0.0
    rows, ts = np.arange(b)[:, None, None], np.arange(TICKS)[None, :, None]
    assert (plan[rows, ts, res['tokens']] != 0).all()
    fol = follow64_plan(Stepper64(params64(make_decoder(hid, vocab, layers)), codes(b), w), res['parents'], res['tokens'], res['finite'], w, plan)
    check_history_plan(fol, res['parents'], res['tokens'], res['scores'], plan, w)


# ---------------------------------------------------------------- 3. the library's new entry points without a GPU
@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _err(lib):
    return lib.arvae_last_error_string().decode()


P = ctypes.c_void_p(256)                                       # never dereferenced: every call below fails validation first
BAD_PLANS = [(dict(allow=None), 'null plan mask'), (dict(row_stride=7), 'row stride'), (dict(row_stride=24 * 35 + 1), 'row stride'),
             (dict(tick_stride=1), 'tick stride'), (dict(tick_stride=36), 'tick stride'), (dict(row_stride=-840), 'row stride')]


def _plan(allow=P, row_stride=24 * 35, tick_stride=35):
    return _lib.NotePlan(allow, row_stride, tick_stride)


def test_tick_free_run_planned_rejects_bad_arguments(lib):
    tw = _lib.TickWeights(*([P] * 8))
    tok = (ctypes.c_int64 * 64)()

    def call(plan=True, top_k=3, top_p=0.9, fallow=None, uniforms=P, inv_t=1.0, ws=P, hidden=128, vocab=35, mask=None, flt=True, **pkw):
        f, n = _lib.SampleFilter(top_k, top_p, fallow), _plan(**pkw)
        return lib.arvae_tick_free_run_planned(ctypes.byref(tw), P, P, 0, P, P, mask, 1.0, 1, 4, 6, hidden, vocab, uniforms, inv_t,
                                               ctypes.byref(f) if flt else None, ctypes.byref(n) if plan else None,
                                               ctypes.cast(tok, ctypes.c_void_p), ws, None)
    assert call(plan=False) == -1 and 'tick_free_run_planned' in _err(lib) and 'null plan' in _err(lib)
    for kw, word in BAD_PLANS:
        assert call(**kw) == -1 and word in _err(lib), kw
    for good in (dict(row_stride=0), dict(tick_stride=0), dict(row_stride=0, tick_stride=0)):           # broadcast strides pass the plan's check: the next one fails
        assert call(ws=None, **good) == -1 and 'workspace' in _err(lib)
    assert call(mask=P) == -1 and 'keep-mask' in _err(lib) and 'plan' in _err(lib)
    assert call(fallow=P) == -1 and 'folded into the plan' in _err(lib)
    assert call(flt=False) == -1 and 'null filter' in _err(lib)
    assert call(top_k=36) == -1 and 'top_k' in _err(lib) and call(top_p=1.5) == -1 and 'top_p' in _err(lib)
    assert call(uniforms=None) == -1 and 'null uniforms' in _err(lib)
    for bad in (0.0, -1.0, float('nan')):
        assert call(inv_t=bad) == -1 and 'inverse temperature' in _err(lib)
    assert call(hidden=48) == -1 and call(hidden=32, vocab=35) == -1          # as arvae_tick_free_run


def test_tick_free_run_layers_planned_rejects_bad_arguments(lib):
    tok = (ctypes.c_int64 * 24)()

    def stack(layers):
        s = _lib.TickStack()
        s.layers = layers
        for l in range(min(layers, 4)):
            s.w_ih[l], s.w_hh[l], s.b_ih[l], s.b_hh[l], s.h0[l] = 256, 256, 256, 256, 256
        s.w_out, s.b_out = 256, 256
        return s

    def call(s, plan=True, uniforms=P, ws=P, hidden=64, mask=None, **pkw):
        f, n = _lib.SampleFilter(3, 0.9, None), _plan(**pkw)
        return lib.arvae_tick_free_run_layers_planned(ctypes.byref(s), P, P, mask, 1.0, 1, 4, 6, hidden, 35, uniforms, 1.0, ctypes.byref(f),
                                                      ctypes.byref(n) if plan else None, ctypes.cast(tok, ctypes.c_void_p), ws, None)
    assert call(stack(3), plan=False) == -1 and 'tick_free_run_layers_planned' in _err(lib) and 'null plan' in _err(lib)
    for kw, word in BAD_PLANS:
        assert call(stack(3), **kw) == -1 and word in _err(lib), kw
    assert call(stack(3), mask=P) == -1 and 'keep-mask' in _err(lib)
    assert call(stack(3), uniforms=None) == -1 and 'null uniforms' in _err(lib)
    assert call(stack(3), ws=None) == -1 and 'workspace' in _err(lib)
    assert call(stack(2)) == -1 and 'arvae_tick_free_run' in _err(lib)
    assert call(stack(3), hidden=128) == -1 and 'not offered' in _err(lib)


def test_tick_by_tick_planned_entry_points_reject_bad_arguments(lib):
    def sample(plan=True, w=P, u=P, out=P, ticks=24, tick=3, fallow=None, inv_t=1.0, **pkw):
        f, n = _lib.SampleFilter(3, 0.9, fallow), _plan(**pkw)
        return lib.arvae_row_sample_planned(w, 2, 35, u, inv_t, ctypes.byref(f), ctypes.byref(n) if plan else None, ticks, tick, out, None)

    def select(plan=True, logits=P, width=4, live=4, ticks=24, tick=3, **pkw):
        n = _plan(**pkw)
        return lib.arvae_beam_select_planned(logits, P, 2, width, 35, live, ctypes.byref(n) if plan else None, ticks, tick, P, P, P, None)

    def score(plan=True, w=P, steps=24, **pkw):
        n = _plan(**pkw)
        return lib.arvae_sequence_log_prob_planned(w, P, 3, steps, 35, ctypes.byref(n) if plan else None, P, None)
    for call, name in ((sample, 'row_sample_planned'), (select, 'beam_select_planned'), (score, 'sequence_log_prob_planned')):
        assert call(plan=False) == -1 and name in _err(lib) and 'null plan' in _err(lib)
        for kw, word in BAD_PLANS:
            assert call(**kw) == -1 and name in _err(lib) and word in _err(lib), (name, kw)
    for call in (sample, select):
        for tick in (-1, 24, 100):
            assert call(tick=tick) == -1 and 'tick' in _err(lib) and '[0, 24)' in _err(lib)
    assert sample(w=None) == -1 and sample(u=None) == -1 and sample(out=None) == -1
    assert sample(fallow=P) == -1 and 'folded into the plan' in _err(lib)
    assert sample(inv_t=0.0) == -1 and 'inverse temperature' in _err(lib)
    assert select(logits=None) == -1 and 'null pointer' in _err(lib)
    for width in (0, 17):
        assert select(width=width, live=1) == -1 and '[1, 16]' in _err(lib)
    for live in (0, 5):
        assert select(live=live) == -1 and 'live' in _err(lib)
    assert score(w=None) == -1 and 'null pointer' in _err(lib)
    assert score(steps=0) == -1 and 'steps' in _err(lib)
    assert score(steps=12) == -1 and 'row stride' in _err(lib)            # the dense stride of another tick count


def test_tick_beam_search_planned_rejects_bad_arguments(lib):
    tw = _lib.TickWeights(*([P] * 8))

    def call(plan=True, weights=tw, width=4, hidden=64, vocab=35, beats=4, ws=P, parents=P, **pkw):
        n = _plan(**pkw)
        return lib.arvae_tick_beam_search_planned(ctypes.byref(weights), P, P, 0, P, P, 3, beats, 6, hidden, vocab, width,
                                                  ctypes.byref(n) if plan else None, parents, P, P, P, P, ws, None)
    assert call(plan=False) == -1 and 'tick_beam_search_planned' in _err(lib) and 'null plan' in _err(lib)
    for kw, word in BAD_PLANS:
        assert call(**kw) == -1 and word in _err(lib), kw
    for width in (0, 17, -3):
        assert call(width=width) == -1 and 'width' in _err(lib) and '[1, 16]' in _err(lib)
    assert call(parents=None) == -1 and 'null output pointer' in _err(lib)
    assert call(ws=None) == -1 and 'workspace' in _err(lib)
    assert call(hidden=48) == -1 and 'hidden size 48' in _err(lib)
    assert call(beats=6, row_stride=36 * 35) == -1 and 'ticks' in _err(lib)
    assert call(hidden=32) == -1 and 'vocab' in _err(lib)


NAMES = ('arvae_row_sample_planned', 'arvae_tick_free_run_planned', 'arvae_tick_free_run_layers_planned', 'arvae_beam_select_planned',
         'arvae_sequence_log_prob_planned', 'arvae_tick_beam_search_planned')


def test_new_entry_points_are_bound_and_declared_once(lib):
    header = open(os.path.join(ROOT, 'include', 'arvae_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(re.findall(r'^int ' + name + r'\(', header, re.M)) == 1, name
    assert len(re.findall(r'^} arvae_note_plan_t;', header, re.M)) == 1


def test_note_plan_struct_matches_the_header(tmp_path):
    """sizeof / field offsets of arvae_note_plan_t as gcc lays it out == the ctypes mirror"""
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('gcc not available')
    fields = ['allow', 'row_stride', 'tick_stride']
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/arvae_hip.h"', 'int main(void) {',
             r'printf("%zu\n", sizeof(arvae_note_plan_t));']
    lines += [rf'printf("%zu\n", offsetof(arvae_note_plan_t, {f}));' for f in fields] + ['return 0; }']
    src = tmp_path / 'sizes.c'
    src.write_text('\n'.join(lines))
    subprocess.run([gcc, '-o', str(tmp_path / 'sizes'), str(src)], check=True)
    out = subprocess.run([str(tmp_path / 'sizes')], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.NotePlan)
    assert [int(v) for v in out[1:]] == [getattr(_lib.NotePlan, f).offset for f in fields]


# ---------------------------------------------------------------- 4. the host side
def test_note_plan_validator():
    _, model, _ = _model_and_trainer()
    dec, v = model.decoder, 35
    assert dec.note_plan(None, 3) is None
    assert dec.note_plan(np.ones((24, v), bool), 3) is None               # all ones: the call without a plan
    assert dec.note_plan(torch.ones(3, 24, v, dtype=torch.int32), 3) is None
    plan = make_plan(3, v)
    got = dec.note_plan(plan, 3)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 24, v) and got.device.type == 'cpu' and got.is_contiguous()
    np.testing.assert_array_equal(got.numpy(), plan)
    shared = dec.note_plan(plan[2].astype(bool), 5)                       # (24, V): the same plan for every row
    assert tuple(shared.shape) == (5, 24, v) and all(np.array_equal(shared[i].numpy(), plan[2]) for i in range(5))
    assert np.array_equal(dec.note_plan(plan.tolist(), 3).numpy(), plan)
    # intersected with `allowed`
    allowed = np.ones(v, np.uint8)
    allowed[1::2] = 0
    both = dec.note_plan(plan[1:3], 2, allowed)
    np.testing.assert_array_equal(both.numpy(), plan[1:3] & allowed)
    with pytest.raises(ValueError, match=r'no note at \(row, tick\) \(0, '):
        dec.note_plan(plan, 3, np.eye(v, dtype=np.uint8)[(plan[0, 0].argmax() + 1) % v])      # the forced note of (0, 0) is not allowed
    empty = plan.copy()
    empty[1, 7] = 0
    with pytest.raises(ValueError, match=r'no note at \(row, tick\) \(1, 7\)'):
        dec.note_plan(empty, 3)
    with pytest.raises(ValueError, match='no note at tick 7'):
        dec.note_plan(empty[1], 3)
    with pytest.raises(ValueError, match='`allowed`'):                     # (V,) is not a plan
        dec.note_plan(np.ones(v, np.uint8), 3)
    for shape in ((24,), (23, v), (24, v + 1), (2, 24, v), (3, 24, v, 1)):
        with pytest.raises(ValueError, match='shape'):
            dec.note_plan(np.ones(shape, np.uint8), 3)
    with pytest.raises(TypeError, match='flags'):
        dec.note_plan(np.ones((24, v), np.float32), 3)
    with pytest.raises(ValueError, match='flags'):
        dec.note_plan(np.full((24, v), 2, np.int64), 3)
    # the decode calls validate before anything touches a device
    z = torch.zeros(3, 16)
    for call in (lambda p: dec.generate(z, plan=p), lambda p: dec.generate(z, sampling='argmax', plan=p),
                 lambda p: dec.beam_search(z, 4, plan=p), lambda p: dec.score_tokens(z, torch.zeros(3, 24, dtype=torch.int64), plan=p)):
        with pytest.raises(ValueError, match='no note at'):
            call(empty)
        with pytest.raises(ValueError, match='`allowed`'):
            call(np.ones(v, np.uint8))
    with pytest.raises(ValueError, match='argmax takes the best allowed note'):
        dec.generate(z, sampling='argmax', plan=plan, top_k=3)
    with pytest.raises(ValueError, match='need sampling'):               # without a plan argmax keeps refusing the cuts
        dec.generate(z, sampling='argmax', allowed=allowed)
    with pytest.raises(ValueError, match='top_k'):
        dec.generate(z, plan=plan, top_k=v + 1)
    for width in (0, 17):
        with pytest.raises(ValueError, match='beam_width'):
            dec.beam_search(z, width, plan=plan)
    with pytest.raises(TypeError, match='beam_width'):
        dec.beam_search(z, 2.0, plan=plan)
    with pytest.raises(RuntimeError, match='no CPU fallback'):            # a valid plan: what is missing here is the GPU
        dec.beam_search(z, 16, plan=plan)                                 # (and the width may exceed a tick's allowed notes)
    assert dec._plan is None and dec._filter is None


def test_build_note_plan():
    ds, _, trainer = _model_and_trainer()
    n2i, v = ds.note2index_dicts, 35
    slur, c4, d4, pads = n2i['__'], 10, 12, [n2i[s] for s in ('START', 'END', None)]
    # a hand-written measure: an onset, three slurs, an onset, a slur, a START symbol (not playable), then slurs
    score = np.full((2, 24), slur, np.int64)
    score[0, [0, 4]] = [c4, d4]
    score[0, 6] = pads[0]
    score[1, ::2] = c4
    assert trainer.build_note_plan().shape == (24, v) and bool(trainer.build_note_plan().all())
    play = trainer.build_note_plan(playable=True)
    assert play.dtype == torch.bool and not play[:, pads].any() and play.sum() == 24 * (v - 3)
    # keep (24,) and (n, 24); (n, 1, 24) scores
    keep = np.zeros(24, bool)
    keep[:6] = True
    plan = trainer.build_note_plan(torch.from_numpy(score)[:, None], keep=keep)
    assert plan.shape == (2, 24, v) and (plan[:, :6].sum(-1) == 1).all() and plan[:, 6:].all()
    np.testing.assert_array_equal(plan[:, :6].int().argmax(-1).numpy(), score[:, :6])
    per_row = np.zeros((2, 24), bool)
    per_row[0, 6] = per_row[1, 23] = True
    plan = trainer.build_note_plan(score, keep=per_row, playable=True)
    assert plan[0, 6].sum() == 1 and plan[0, 6, pads[0]]                  # a forced note stands even if it is not playable
    assert plan[1, 23].sum() == 1 and plan[1, 23, score[1, 23]]
    free = np.ones((2, 24), bool) & ~per_row
    assert not plan[free][:, pads].any() and (plan[free].sum(-1) == v - 3).all()
    # keep_rhythm: slurs forced where the score holds them, banned everywhere else
    plan = trainer.build_note_plan(score, keep_rhythm=True)
    at_slur = score == slur
    assert (plan[at_slur].sum(-1) == 1).all() and plan[at_slur][:, slur].all()
    assert not plan[~at_slur][:, slur].any() and (plan[~at_slur].sum(-1) == v - 1).all()
    plan = trainer.build_note_plan(score, keep=keep, keep_rhythm=True, allowed=np.eye(v, dtype=np.uint8)[[slur, c4, d4]].sum(0))
    assert plan[0, 0].sum() == 1 and plan[0, 0, c4] and plan[0, 4, d4] and plan[0, 4].sum() == 1
    assert plan[0, 6].tolist() == [i in (c4, d4) for i in range(v)]       # free, an onset: the allowed notes without the slur
    assert trainer.model.decoder.note_plan(plan, 2) is not None
    for bad in (np.zeros(23, bool), np.zeros((3, 24), bool), np.zeros(24, np.int64)):
        with pytest.raises(ValueError, match='keep must be a bool mask'):
            trainer.build_note_plan(score, keep=bad)
    with pytest.raises(ValueError, match='needs `score`'):
        trainer.build_note_plan(keep=keep)
    with pytest.raises(ValueError, match='score must hold note indices'):
        trainer.build_note_plan(np.zeros((2, 23), np.int64), keep=keep)
    with pytest.raises(ValueError, match='outside'):
        trainer.build_note_plan(np.full((2, 24), v, np.int64), keep=keep)


def test_infill_measures_and_decode_arguments():
    _, _, trainer = _model_and_trainer()
    score = np.zeros((2, 24), np.int64)
    keep = np.zeros(24, bool)
    keep[:6] = True
    with pytest.raises(ValueError, match='sampling must be'):
        trainer.infill_measures(score, keep=keep, sampling='greedy')
    with pytest.raises(ValueError, match='keeps something'):
        trainer.infill_measures(score)
    with pytest.raises(ValueError, match='keep must be a bool mask'):
        trainer.infill_measures(score, keep=np.zeros(5, bool))
    with pytest.raises(ValueError, match="sampling='beam' draws nothing"):
        trainer.infill_measures(score, keep=keep, sampling='beam', top_k=3)
    with pytest.raises(ValueError, match='no note at'):
        trainer.decode_latent_codes(torch.zeros(2, 16), plan=np.zeros((24, 35), np.uint8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):            # valid arguments: what is missing here is the GPU
        trainer.infill_measures(score, keep=keep, keep_rhythm=True, playable=True)


def test_cli_keep_ticks_parser_and_refusals():
    sys.path.insert(0, ROOT)
    import train_measure_vae as cli
    ticks = lambda spec: [t for t, k in enumerate(cli.parse_keep_ticks(spec)) if k]
    assert ticks('0-5,12-17') == list(range(6)) + list(range(12, 18))
    assert ticks('3') == [3] and ticks('23,0') == [0, 23] and ticks(' 1 - 2 , 4') == [1, 2, 4] and ticks('0-23') == list(range(24))
    for bad in ('', ',', '1,,2', 'a', '1-b', '5-2', '24', '0-24', '-3', '1-2-3', '1.5'):
        with pytest.raises(ValueError, match='--keep_ticks'):
            cli.parse_keep_ticks(bad)
    # refused before anything is loaded (main would stop on the missing dataset first)
    for args in (['--infill', '4', '--keep_ticks', '0-30'], ['--infill', '4', '--keep_ticks', 'x'], ['--infill=4', '--keep_ticks=7-3']):
        with pytest.raises(ValueError, match='--keep_ticks'):
            cli.run(args)
    with pytest.raises(ValueError, match='--keep_ticks SPEC or --keep_rhythm'):
        cli.run(['--infill', '4'])
    with pytest.raises(ValueError, match='belong to --infill'):
        cli.run(['--keep_ticks', '0-5'])
    with pytest.raises(ValueError, match='--infill takes a count'):
        cli.run(['--infill', '-1', '--keep_rhythm'])
    with pytest.raises(ValueError, match='--beam'):
        cli.run(['--infill', '4', '--keep_ticks', '0-5', '--beam', '4', '--top_k', '3'])
    assert '--infill' in cli.INFILL_HELP and '--keep_ticks' in cli.INFILL_HELP and '--keep_rhythm' in cli.INFILL_HELP

"""Note plans of the MeasureVAE decoder on the device (include/arvae_hip.h, arvae_note_plan_t): exact properties of every decode mode
under a plan on the one-launch kernels and tick by tick, the planned picks against the weights the whole-sequence kernels return, the
planned beam search step by step against the float64 follower of tests/test_note_plan.py, and infilling through the trainer and the
command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arvae_amd  # noqa: F401
from arvae_amd import ops
from arvae_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_beam_search import DELTA, OTHER_SHAPES, Stepper64, backtrack, codes, make_decoder, params64  # noqa: E402
from test_beam_search_gpu import SCORE_BAR  # noqa: E402
from test_note_plan import (BEAM_CASES, PICK_CASES, PICK_STEPWISE_ONLY, beam_id, check_history_plan, draws, finite_counts,  # noqa: E402
                            follow64_plan, make_plan, pick_id)
from test_sampling import _FolkDataset  # noqa: E402
from test_sampling_filters import check_tick_picks  # noqa: E402
from test_sampling_filters_gpu import EXACT_CASES, _decoder, _half_mask  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _obeys(plan, tokens):
    """tokens (B, 24) or (B, 24, W) lie inside their (row, tick)'s allowed set"""
    tokens = np.asarray(tokens)
    t = tokens if tokens.ndim == 3 else tokens[..., None]
    b, ticks, _ = t.shape
    return bool((plan[np.arange(b)[:, None, None], np.arange(ticks)[None, :, None], t] != 0).all())


# ---------------------------------------------------------------- 5. exact properties, one launch and tick by tick
@pytest.mark.parametrize('mode', ('0', '1'), ids=('one_launch', 'stepwise'))
@pytest.mark.parametrize('case', EXACT_CASES, ids=[f'b{c[0]}_h{c[1]}_v{c[2]}_l{c[3]}' for c in EXACT_CASES])
def test_planned_decoding_exact_properties(dev, monkeypatch, case, mode):
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
    b, hid, vocab, layers = case
    assert ops.tick_free_run_supported(hid, vocab) if layers == 2 else ops.tick_free_run_layers_supported(hid, vocab, layers)
    dec = _decoder(hid, vocab, layers)
    z = torch.from_numpy(syn.normal_noise((b, 32), seed=29)).to(dev)
    u = draws(b, edges=True)                                              # a third of the rows draw u = 1 throughout, row 1 draws 2^-32
    ut = torch.from_numpy(u)
    plan = make_plan(b, vocab)
    forced = plan[0].argmax(-1)                                           # row 0's measure
    ones = np.ones((b, 24, vocab), np.uint8)
    mask = _half_mask(vocab)
    mask[0] = 0
    rep = np.ascontiguousarray(np.broadcast_to(mask, (b, 24, vocab)))
    w = 4
    cuts = ({}, {'top_k': 3}, {'top_p': 0.7}, {'top_k': 5, 'top_p': 0.8})
    # a plan of all ones is the call without a plan; a plan that repeats one mask is allowed = that mask: bit for bit
    for kw in cuts:
        plain = dec.generate(z, uniforms=ut, temperature=0.8, **kw)[1]
        assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, plan=ones, **kw)[1], plain), kw
        masked = dec.generate(z, uniforms=ut, temperature=0.8, allowed=mask, **kw)[1]
        assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, plan=rep, **kw)[1], masked), kw
        assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, plan=rep[0], **kw)[1], masked), kw       # (24, V): every row
        assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, plan=ones, allowed=mask, **kw)[1], masked), kw
    greedy = dec.generate(z, sampling='argmax')[1]
    assert torch.equal(dec.generate(z, sampling='argmax', plan=ones)[1], greedy)
    for a, b_ in zip(dec.beam_search(z, w, plan=ones, return_history=True), dec.beam_search(z, w, return_history=True)):
        assert all(torch.equal(x, y) for x, y in zip(a, b_)) if isinstance(a, tuple) else torch.equal(a, b_)
    for a, b_ in zip(dec.beam_search(z, w, plan=rep, return_history=True), dec.beam_search(z, w, allowed=mask, return_history=True)):
        assert all(torch.equal(x, y) for x, y in zip(a, b_)) if isinstance(a, tuple) else torch.equal(a, b_)
    seq = dec.beam_search(z, w, allowed=mask)[1]
    assert torch.equal(dec.score_tokens(z, seq, plan=ones), dec.score_tokens(z, seq))
    assert torch.equal(dec.score_tokens(z, seq, plan=rep), dec.score_tokens(z, seq, allowed=mask))
    assert bool(torch.isfinite(dec.score_tokens(z, seq, plan=rep)).all())
    # the random plan: no emitted note outside its A(b, t) in any mode, row 0 reproduces its forced measure in every mode
    outs = []
    for tau in (0.8, 1.3):
        for kw in cuts:
            outs.append(dec.generate(z, uniforms=ut, temperature=tau, plan=plan, **kw)[1][:, 0].cpu().numpy())
    before = ops.RngState.offset
    weights, best = dec.generate(z, sampling='argmax', plan=plan)
    assert ops.RngState.offset == before                                  # the planned argmax consumes no draw
    assert best.shape == (b, 1, 24) and best.dtype == torch.int64 and weights.shape == (b, 24, vocab)
    outs.append(best[:, 0].cpu().numpy())
    for tok in outs:
        assert tok.min() >= 0 and tok.max() < vocab and _obeys(plan, tok)
        np.testing.assert_array_equal(tok[0], forced)
    assert len(np.unique(outs[0])) > 3 and not np.array_equal(outs[0], outs[-1])
    # the planned argmax is the planned draw with top_k = 1, whatever the draws, the other cut and the temperature
    assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, top_k=1, plan=plan)[1], best)
    assert torch.equal(dec.generate(z, uniforms=ut, temperature=1.7, top_k=1, top_p=0.5, plan=plan)[1], best)
    # ... and the best allowed note of the returned weights wherever that one stands clear (the forced note was fed back)
    wn = np.where(plan != 0, weights.double().cpu().numpy(), -1.0)
    top2 = np.sort(wn, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-3
    assert clear.mean() > 0.5
    np.testing.assert_array_equal(outs[-1][clear], wn.argmax(-1)[clear])
    # scoring: 24 forced ticks add exactly 0.0; a token outside its A(b, t) has no probability
    scores = dec.score_tokens(z, best, plan=plan)
    assert scores.shape == (b,) and float(scores[0]) == 0.0 and bool(torch.isfinite(scores).all()) and float(scores[1:].max()) < 0.0
    bad = best[:, 0].clone()
    bad[0, 5] = (int(forced[5]) + 1) % vocab
    again = dec.score_tokens(z, bad, plan=plan)
    assert float(again[0]) == -np.inf and torch.equal(again[1:], scores[1:])
    # beam search: every token of every slot obeys the plan, row 0 ends with its forced measure alone, dead slots last
    res = dec.beam_search(z, w, plan=plan, return_history=True)
    seqs, sc, (parents, tokens, hist) = res[3].cpu().numpy(), res[4].cpu().numpy(), [x.cpu().numpy() for x in res[5]]
    assert _obeys(plan, tokens) and _obeys(plan, seqs.transpose(0, 2, 1))
    np.testing.assert_array_equal(backtrack(parents, tokens), seqs)
    np.testing.assert_array_equal(seqs[0, 0], forced)
    assert sc[0, 0] == 0.0 and (sc[0, 1:] == -np.inf).all() and np.isfinite(sc[1]).all()
    np.testing.assert_array_equal(np.isfinite(hist).sum(-1), finite_counts(plan, w))
    assert (np.diff(np.isfinite(hist).astype(np.int8), axis=-1) <= 0).all() and not np.isnan(hist).any()
    np.testing.assert_array_equal(res[1][:, 0].cpu().numpy(), seqs[:, 0])
    wide = dec.beam_search(z, 16, plan=plan)                              # a width above what many ticks allow is accepted
    assert _obeys(plan, wide[3].cpu().numpy().transpose(0, 2, 1)) and float(wide[4][0, 0]) == 0.0
    assert dec.training and dec.sampling == 'argmax' and dec._filter is None and dec._plan is None and dec.use_teacher_forcing is True


# ---------------------------------------------------------------- 6. picks against the returned weights, both paths
_RUNS = {}


def planned_run(case, mode, dev, monkeypatch):
    """(tokens (b, 24), clear rows) of a case with ARVAE_TICK_STEPWISE = mode, once: every emitted note is the float64 filtered pick
    over its (row, tick)'s allowed set from the returned weights -- the teacher-forced weights on the emitted tokens, so a forced
    note that had not been fed back would show in every later tick (band: eps = 1e-5 max|w| + 1e-6, delta = 2 eps / tau + 1e-5)"""
    if (case, mode) not in _RUNS:
        b, hid, vocab, layers, top_k, top_p, tau = case
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        dec = _decoder(hid, vocab, layers)
        z = torch.from_numpy(syn.normal_noise((b, 32), seed=29)).to(dev)
        u, plan = draws(b), make_plan(b, vocab)
        before = ops.RngState.offset
        out = {}
        for name, kw, (k, p) in (('draw', dict(uniforms=torch.from_numpy(u), temperature=tau, top_k=top_k, top_p=top_p), (top_k, top_p)),
                                 ('argmax', dict(sampling='argmax'), (1, 1.0))):
            weights, samples = dec.generate(z, plan=plan, **kw)
            assert samples.shape == (b, 1, 24) and samples.dtype == torch.int64 and weights.shape == (b, 24, vocab)
            tok = samples[:, 0].cpu().numpy()
            w = weights.double().cpu().numpy()
            eps = 1e-5 * float(np.abs(w).max()) + 1e-6
            delta = 2.0 * eps / tau + 1e-5
            share, clear = check_tick_picks(tok, w, u, tau, plan, k, p, eps, delta)
            print(f'planned {name} case {pick_id(case)} stepwise {mode}: delta {delta:.3e}, ambiguous draws {share:.5f}, '
                  f'distinct notes {len(np.unique(tok))}')
            assert share <= 0.05                                          # beyond that the test proves nothing
            assert len(np.unique(tok)) > 3 and _obeys(plan, tok)
            np.testing.assert_array_equal(tok[0], plan[0].argmax(-1))
            out[name] = (tok, clear.all(1))
        assert ops.RngState.offset == before                              # every draw was an explicit input, the argmax drew nothing
        _RUNS[(case, mode)] = out
    return _RUNS[(case, mode)]


@pytest.mark.parametrize('case', PICK_CASES, ids=[pick_id(c) for c in PICK_CASES])
def test_planned_kernel_samples_its_own_weights(dev, monkeypatch, case):
    planned_run(case, '0', dev, monkeypatch)


@pytest.mark.parametrize('case', PICK_CASES, ids=[pick_id(c) for c in PICK_CASES])
def test_per_tick_path_picks_the_same_planned_notes(dev, monkeypatch, case):
    """ARVAE_TICK_STEPWISE=1 (arvae_row_sample_planned per tick) passes the same check, and rows without an ambiguous draw in either
    mode carry identical notes in both"""
    step, fast = planned_run(case, '1', dev, monkeypatch), planned_run(case, '0', dev, monkeypatch)
    for name in ('draw', 'argmax'):
        both = fast[name][1] & step[name][1]
        assert both.mean() > 0.5
        np.testing.assert_array_equal(fast[name][0][both], step[name][0][both])


@pytest.mark.parametrize('case', PICK_STEPWISE_ONLY, ids=[pick_id(c) for c in PICK_STEPWISE_ONLY])
def test_shapes_without_a_one_launch_kernel_follow_the_plan_tick_by_tick(dev, monkeypatch, case):
    _, hid, vocab, layers = case[:4]
    assert not (ops.tick_free_run_supported(hid, vocab) if layers == 2 else ops.tick_free_run_layers_supported(hid, vocab, layers))
    planned_run(case, '0', dev, monkeypatch)


# ---------------------------------------------------------------- 7. beam search under the plan against the float64 follower
_BEAMS = {}


def beam_run(case, mode, dev, monkeypatch):
    """one planned beam search of a case with ARVAE_TICK_STEPWISE = mode, its float64 follower and its checks, once -> the run"""
    if (case, mode) not in _BEAMS:
        b, hid, vocab, layers, w = case
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        dec = make_decoder(hid, vocab, layers).cuda()
        z = torch.from_numpy(codes(b)).to(dev)
        plan = make_plan(b, vocab)
        weights, samples, best, seqs, scores, (parents, tokens, hist) = dec.beam_search(z, w, plan=plan, return_history=True)
        assert weights.shape == (b, 24, vocab) and samples.shape == (b, 1, 24) and best.shape == (b,)
        assert seqs.shape == (b, w, 24) and seqs.dtype == torch.int64 and scores.shape == (b, w) and scores.dtype == torch.float32
        assert parents.shape == tokens.shape == hist.shape == (b, 24, w) and parents.dtype == torch.int32
        run = dict(seqs=seqs.cpu().numpy(), scores=scores.cpu().numpy(), parents=parents.cpu().numpy(), tokens=tokens.cpu().numpy(),
                   hist=hist.cpu().numpy(), plan=plan)
        np.testing.assert_array_equal(backtrack(run['parents'], run['tokens']), run['seqs'])
        np.testing.assert_array_equal(run['scores'], run['hist'][:, -1])
        np.testing.assert_array_equal(samples[:, 0].cpu().numpy(), run['seqs'][:, 0])
        finite = np.isfinite(run['hist'])
        fol = follow64_plan(Stepper64(params64(dec), codes(b), w), run['parents'], run['tokens'], finite, w, plan)
        share, clear = check_history_plan(fol, run['parents'], run['tokens'], run['hist'], plan, w)
        err_hist = float(np.abs(np.where(finite, run['hist'] - np.where(finite, fol['chosen'], 0.0), 0.0)).max())
        # the final count, in integer arithmetic; dead slots -inf, last, inside the plan (check_history_plan: every tick's)
        want = [min(w, int(np.prod([int(n) for n in (plan[row] != 0).sum(-1)], dtype=object))) for row in range(b)]
        np.testing.assert_array_equal(np.isfinite(run['scores']).sum(1), want)
        assert want[0] == 1 and want[1] == w
        np.testing.assert_array_equal(run['seqs'][0, 0], plan[0].argmax(-1))
        assert run['scores'][0, 0] == 0.0
        ts = np.arange(24)
        for j in range(w):
            assert (plan[np.arange(b)[:, None], ts[None, :], run['seqs'][:, j]] != 0).all()
        # the best beam's score is the planned log-probability of its tokens
        again = dec.score_tokens(z, seqs[:, 0].contiguous(), plan=plan).cpu().numpy()
        err_seq = float(np.abs(again - run['scores'][:, 0]).max())
        print(f'planned beam case {beam_id(case)} stepwise {mode}: ambiguous steps {share:.4f}, |scores - float64| {err_hist:.3e}, '
              f'|scores - score_tokens| {err_seq:.3e} (bar {SCORE_BAR:.1e})')
        assert share <= 0.05                                              # beyond that the test proves nothing
        assert err_seq <= SCORE_BAR
        assert dec.training and dec.use_teacher_forcing is True and dec._plan is None
        run['clear'] = clear
        _BEAMS[(case, mode)] = run
    return _BEAMS[(case, mode)]


@pytest.mark.parametrize('case', BEAM_CASES, ids=[beam_id(c) for c in BEAM_CASES])
def test_planned_beam_selection_vs_float64(dev, monkeypatch, case):
    assert case[3] != 2 or ops.tick_beam_search_supported(case[1], case[2], case[4])     # two layers: the one-launch kernel
    beam_run(case, '0', dev, monkeypatch)


@pytest.mark.parametrize('case', [c for c in BEAM_CASES if c[3] == 2], ids=[beam_id(c) for c in BEAM_CASES if c[3] == 2])
def test_tick_by_tick_path_selects_the_same_planned_beams(dev, monkeypatch, case):
    """ARVAE_TICK_STEPWISE=1 (arvae_beam_select_planned per tick) passes the same checks, and codes without an ambiguous step on
    either path carry identical finite histories on both"""
    step, fast = beam_run(case, '1', dev, monkeypatch), beam_run(case, '0', dev, monkeypatch)
    both = fast['clear'].all(1) & step['clear'].all(1)
    assert both.mean() > 0.3
    fin = np.isfinite(fast['hist'])
    np.testing.assert_array_equal(fin, np.isfinite(step['hist']))
    sel = both[:, None, None] & fin
    np.testing.assert_array_equal(fast['parents'][sel], step['parents'][sel])
    np.testing.assert_array_equal(fast['tokens'][sel], step['tokens'][sel])
    assert np.abs(fast['hist'][sel] - step['hist'][sel]).max() <= SCORE_BAR


@pytest.mark.parametrize('case', OTHER_SHAPES, ids=[beam_id(c) for c in OTHER_SHAPES])
def test_shapes_without_a_one_launch_beam_kernel_follow_the_plan(dev, monkeypatch, case):
    assert not ops.tick_beam_search_supported(case[1], case[2], case[4])
    beam_run(case, '0', dev, monkeypatch)


# ---------------------------------------------------------------- 8. the trainer and the command line
KEEP_SPEC = '0-5,12-17'                                        # beats 0 and 2


def test_trainer_infills_measures(dev):
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    torch.manual_seed(0)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.5, 16, 2, 64, 0.5, False, 'folk')
    trainer = MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))
    trainer.cuda()
    model.eval()
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
    slur = ds.note2index_dicts['__']
    pads = [ds.note2index_dicts[s] for s in ('START', 'END', None)]
    score = syn.measure_batch(12, seed=3)
    keep = np.zeros(24, bool)
    keep[:6] = keep[12:18] = True
    free_out = []
    for sampling, kw in (('argmax', {}), ('multinomial', dict(temperature=0.9, top_k=5, top_p=0.9)), ('beam', dict(beam_width=4))):
        none, notes = trainer.infill_measures(score, keep=keep, sampling=sampling, playable=True, **kw)
        assert none is None and notes.shape == (12, 1, 24) and notes.dtype == torch.int64
        got = notes[:, 0].cpu().numpy()
        np.testing.assert_array_equal(got[:, keep], score[:, keep])       # the kept ticks come back as they were
        assert not np.isin(got[:, ~keep], pads).any()                     # the rewritten ones are playable
        free_out.append(got[:, ~keep])
        _, notes = trainer.infill_measures(score, keep=keep, keep_rhythm=True, sampling=sampling, **kw)
        got = notes[:, 0].cpu().numpy()
        np.testing.assert_array_equal(got[:, keep], score[:, keep])
        np.testing.assert_array_equal(got == slur, score == slur)         # '__' exactly where the input has it
        _, notes = trainer.infill_measures(torch.from_numpy(score)[:, None], keep_rhythm=True, sampling=sampling, **kw)
        np.testing.assert_array_equal(notes[:, 0].cpu().numpy() == slur, score == slur)
    assert any(not np.array_equal(free_out[0], o) for o in free_out[1:])   # the modes do write different notes
    # a plan through decode_latent_codes, per row
    z = torch.randn(12, 16).to(dev)
    plan = trainer.build_note_plan(score, keep=keep, playable=True)
    for sampling in ('argmax', 'multinomial', 'beam'):
        _, notes = trainer.decode_latent_codes(z, sampling=sampling, plan=plan)
        np.testing.assert_array_equal(notes[:, 0].cpu().numpy()[:, keep], score[:, keep])
    assert not model.training and model.decoder.sampling == 'argmax' and model.decoder._plan is None


def test_cli_infill_flags(dev, tmp_path):
    """--infill 4 --keep_ticks 0-5,12-17 --playable after a short synthetic run, and once more with --beam 4 on the saved model: both
    print four original and four infilled measures whose kept ticks agree and whose rewritten ticks hold no padding symbol"""
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    common = ['--infill', '4', '--keep_ticks', KEEP_SPEC, '--playable', '--batch_size', '16', '--rand', '1', '-r', 'all',
              '--encoder_hidden_size', '64', '--decoder_hidden_size', '64']
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(tmp_path / 'models'))
    kept = list(range(6)) + list(range(12, 18))
    for extra, mode in ((['--num_epochs', '1'], 'argmax'), (['--test', '--beam', '4'], 'beam')):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + extra + common, capture_output=True, text=True,
                           timeout=600, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        summary = json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]
        infill = summary['infill']
        assert infill['sampling'] == mode and infill['keep_ticks'] == kept and infill['playable'] is True and infill['keep_rhythm'] is False
        assert len(infill['original']) == len(infill['infilled']) == 4
        for old, new in zip(infill['original'], infill['infilled']):
            assert len(old) == len(new) == 24 and set(new) <= set(n2i)
            assert [new[t] for t in kept] == [old[t] for t in kept]
            assert not {new[t] for t in range(24) if t not in kept} & {'START', 'END', None, 'None'}

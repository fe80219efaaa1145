"""Diverse beam search of the MeasureVAE decoder on the device (include/arvae_hip.h, "Diverse beam search"): exact properties of the
histories, the grouped selection step by step against the float64 follower of tests/test_diverse_beam.py, scores and log_probs against
the measured bar of tests/test_beam_search_gpu.py, the one-launch kernel against the tick-by-tick path, the trainer and the command
line."""
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
from test_beam_search import Stepper64, backtrack, codes, make_decoder, params64  # noqa: E402
from test_beam_search_gpu import SCORE_BAR  # noqa: E402
from test_diverse_beam import CASES, LAMBDA, VARIANTS, admits, case_id, check_groups, dfollow64, variant_plan  # noqa: E402
from test_note_plan import finite_counts  # noqa: E402
from test_sampling import _FolkDataset  # noqa: E402

TWO_LAYER = [c for c in CASES if c[3] == 2 and c[1] in (32, 64, 128) and c[2] <= 64]
# (case, ARVAE_TICK_STEPWISE): both paths where a one-launch kernel exists, else the one there is
CASE_MODES = [(c, m) for c in CASES for m in (('0', '1') if c in TWO_LAYER else ('0',))]
# (case, variant): the variants a case admits (tests/test_diverse_beam.py)
CASE_VARIANTS = [(c, v) for c in CASES for v in VARIANTS if admits(c, v)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def clear_prefix(clear):
    """clear (B, T, G) -> (B, T): the ticks of a code up to its first ambiguous selection.  Before it float64 leaves no choice, so
    two device runs of the code must carry the same history there; a code clear throughout is clear at all 24."""
    return np.logical_and.accumulate(clear.all(2), axis=1)


def one_launch(case):
    return case[3] == 2 and ops.tick_beam_search_groups_supported(case[1], case[2], case[4], case[5])


def search_kwargs(case, variant):
    """the allowed notes of a variant the way a caller gives them: nothing, a mask, a plan"""
    from test_beam_search import half_mask
    if variant == 'free':
        return {}
    if variant == 'half':
        return {'allowed': half_mask(case[2])}
    return {'plan': variant_plan(case, variant)}


_DECS, _RUNS = {}, {}


def decoder(case):
    key = case[1:4]
    if key not in _DECS:
        _DECS[key] = make_decoder(*key).cuda()
    return _DECS[key]


def search(case, mode, variant, dev, monkeypatch, lam=LAMBDA, width=None, groups=None, z=None):
    """one diverse search of a case with ARVAE_TICK_STEPWISE = mode -> dict of numpy arrays (and the device sequences)"""
    b, hid, vocab, layers, w, g = case
    w, g = w if width is None else width, g if groups is None else groups
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
    dec = decoder(case)
    z = torch.from_numpy(codes(b)).to(dev) if z is None else z
    n = z.shape[0]
    weights, samples, best, seqs, scores, logp, (parents, tokens, hist) = dec.beam_search(
        z, w, return_history=True, beam_groups=g, diversity=lam, **search_kwargs(case, variant))
    assert dec.training and dec.use_teacher_forcing is True and dec.sampling == 'argmax' and dec._filter is None and dec._plan is None
    assert weights.shape == (n, 24, vocab) and samples.shape == (n, 1, 24) and samples.dtype == torch.int64 and best.shape == (n,)
    assert seqs.shape == (n, w, 24) and seqs.dtype == torch.int64
    assert scores.shape == logp.shape == (n, w) and scores.dtype == logp.dtype == torch.float32
    assert parents.shape == tokens.shape == hist.shape == (n, 24, w)
    assert parents.dtype == torch.int32 and tokens.dtype == torch.int64 and hist.dtype == torch.float32
    return dict(dec=dec, z=z, samples=samples[:, 0].cpu().numpy(), best=best.cpu().numpy(), seqs=seqs.cpu().numpy(),
                scores=scores.cpu().numpy(), logp=logp.cpu().numpy(), parents=parents.cpu().numpy(), tokens=tokens.cpu().numpy(),
                hist=hist.cpu().numpy(), seqs_dev=seqs)


def run_of(case, mode, variant, dev, monkeypatch):
    """the case's search at LAMBDA and its float64 follower, once per (case, mode, variant)"""
    key = (case, mode, variant)
    if key not in _RUNS:
        b, hid, vocab, layers, w, g = case
        run = search(case, mode, variant, dev, monkeypatch)
        run['plan'] = variant_plan(case, variant)
        run['fol'] = dfollow64(Stepper64(params64(run['dec']), codes(b), w), run['parents'], run['tokens'], np.isfinite(run['hist']), w, g,
                               LAMBDA, run['plan'])
        # `clear` (the W'-th against the (W'+1)-th key) is what the ambiguous share counts; histories of two device runs are compared
        # where the selections were also `ordered`: no two picks of a list closer than twice the bar the keys are held to
        run['share'], run['clear'], run['ordered'] = check_groups(run['fol'], run['parents'], run['tokens'], run['hist'], run['plan'], w, g,
                                                                  order_bar=2.0 * SCORE_BAR)
        _RUNS[key] = run
    return _RUNS[key]


# ---------------------------------------------------------------- 1. exact, oracle-free
@pytest.mark.parametrize('case,mode', CASE_MODES, ids=[f'{case_id(c)}_stepwise{m}' for c, m in CASE_MODES])
def test_diverse_histories_exact_properties(dev, monkeypatch, case, mode):
    b, hid, vocab, layers, w, g = case
    wg = w // g
    assert one_launch(case) == (case in TWO_LAYER)
    run = run_of(case, mode, 'free', dev, monkeypatch)
    np.testing.assert_array_equal(backtrack(run['parents'], run['tokens']), run['seqs'])
    np.testing.assert_array_equal(run['samples'], run['seqs'][:, 0])
    np.testing.assert_array_equal(run['best'], run['scores'][:, 0])
    np.testing.assert_array_equal(run['scores'], run['hist'][:, -1])
    assert run['tokens'].min() >= 0 and run['tokens'].max() < vocab
    assert (run['parents'] // wg == np.arange(w) // wg).all()             # a parent is a beam of the same group
    assert (run['parents'][:, 0] == np.arange(w) // wg * wg).all()        # tick 0: the group's first beam
    assert np.isfinite(run['hist']).all() and np.isfinite(run['logp']).all()
    for i in range(g):
        sl = slice(i * wg, (i + 1) * wg)
        assert (np.diff(run['hist'][..., sl], axis=-1) <= 0).all()
        for code in range(b):
            assert len({tuple(s) for s in run['seqs'][code, sl]}) == wg, (code, i)
    assert (run['scores'] <= run['logp']).all() and (run['scores'][:, :wg] == run['logp'][:, :wg]).all()       # group 0 never pays
    # penalty 0: all groups of a code are bit-identical, and the scores are the log-probabilities bit for bit
    flat = search(case, mode, 'free', dev, monkeypatch, lam=0.0)
    for key in ('tokens', 'hist'):
        for i in range(1, g):
            np.testing.assert_array_equal(flat[key][..., i * wg:(i + 1) * wg], flat[key][..., :wg])
    for i in range(1, g):
        np.testing.assert_array_equal(flat['parents'][..., i * wg:(i + 1) * wg], flat['parents'][..., :wg] + i * wg)
        np.testing.assert_array_equal(flat['seqs'][:, i * wg:(i + 1) * wg], flat['seqs'][:, :wg])
    assert (flat['scores'].view(np.int32) == flat['logp'].view(np.int32)).all()
    # one group, and group 0 at LAMBDA, are the search of width W' without groups: identical histories wherever no ambiguous step
    # has come yet (so at every tick of a code without one), scores within the bar everywhere
    dec, z = run['dec'], run['z']
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
    plain = dec.beam_search(z, wg, return_history=True)
    pp, pt, ph = (x.cpu().numpy() for x in plain[5])
    rows = clear_prefix(run['ordered'][:, :, :1])                           # (B, T): group 0's ticks before its first ambiguous one
    assert rows.mean() > 0.3
    single = search(case, mode, 'free', dev, monkeypatch, width=wg, groups=1)
    for got in (single, {k: (v[..., :wg] if k in ('parents', 'tokens', 'hist') else v) for k, v in run.items()}):
        np.testing.assert_array_equal(got['parents'][rows], pp[rows])
        np.testing.assert_array_equal(got['tokens'][rows], pt[rows])
        assert np.abs(got['hist'] - ph).max() <= SCORE_BAR
        assert np.abs(got['logp'][:, :wg] - plain[4].cpu().numpy()).max() <= SCORE_BAR
    # beams of a ragged tail never leak into live codes: the same codes in a batch that fills the tiles
    full = -(-b // 16) * 16 + 16
    zf = torch.cat((z, torch.from_numpy(syn.normal_noise((full - b, 32), seed=31)).to(dev)), 0)
    filled = search(case, mode, 'free', dev, monkeypatch, z=zf)
    pre = clear_prefix(run['ordered'])                                    # (a code clear at every tick is compared at every tick)
    print(f'diverse beam case {case_id(case)} mode {mode}: codes clear throughout {run["ordered"].all((1, 2)).mean():.3f}, ticks before '
          f'the first ambiguous selection {pre.mean():.3f}')
    assert pre.mean() > 0.3
    np.testing.assert_array_equal(filled['parents'][:b][pre], run['parents'][pre])
    np.testing.assert_array_equal(filled['tokens'][:b][pre], run['tokens'][pre])
    assert np.abs(filled['hist'][:b][pre] - run['hist'][pre]).max() <= SCORE_BAR


def test_penalised_key_rounds_the_product_and_the_difference(dev):
    """a = c - penalty * float(n) with the product rounded before the difference -- not fma(-penalty, n, c) --, bit for bit, on both
    kernels.  W = G = 4 on logits whose note 0 stands 10 above the rest: groups 0 to 2 take note 0, so group 3 keys it with n = 3
    (n <= 2 and the penalties 0 and 0.5 of the other tests make the product exact and cannot tell the two apart).  Group 0's score is
    the device's own c (every beam has the same logits and score 0); over 64 penalties the written definition and the fused form
    differ in the last bit for some, and the device gives the written one for all."""
    vocab, three = 35, np.float32(3.0)
    logits = np.zeros((4, vocab), np.float32)
    logits[:, 0] = 10.0
    args = (torch.from_numpy(logits).to(dev), torch.zeros(1, 4, device=dev), torch.zeros(1, 4, device=dev), 1, 4)
    mask = torch.ones(vocab, dtype=torch.uint8, device=dev)
    told_apart = 0
    for i in range(64):
        lam = np.float32(0.1 + 0.013 * i)
        par, note, score, logp = ops.beam_select_groups(*args, float(lam), mask, 0, ticks=1)
        assert note.cpu().tolist() == [[0, 0, 0, 0]] and par.cpu().tolist() == [[0, 1, 2, 3]]
        s = score.cpu().numpy()[0]
        c = s[0]
        assert (logp.cpu().numpy()[0] == c).all()
        written = np.float32(c - np.float32(lam * three))                 # fp32 product, fp32 difference
        fused = np.float32(np.float64(c) - np.float64(lam) * 3.0)         # one rounding (exact in float64: 24 + 2 bits)
        assert s[1] == np.float32(c - lam) and s[2] == np.float32(c - np.float32(lam * np.float32(2.0)))
        assert s[3] == written, (float(lam), float(s[3]), float(written), float(fused))
        told_apart += int(written != fused)
    assert told_apart > 0
    # the one-launch kernel: a decoder whose every logit but note 0's is zero, so that all four groups take note 0 at tick 0
    dec = make_decoder(64, 35, 2).cuda()
    with torch.no_grad():
        dec.tick_emb_to_note_emb[0].weight.zero_()
        dec.tick_emb_to_note_emb[0].bias.zero_()
        dec.tick_emb_to_note_emb[0].bias[0] = 10.0
    z = torch.from_numpy(codes(3)).to(dev)
    told_apart = 0
    for i in range(16):
        lam = np.float32(0.1 + 0.053 * i)
        hist = dec.beam_search(z, 4, beam_groups=4, diversity=float(lam), return_history=True)[6][2][:, 0].cpu().numpy()
        c = hist[:, 0]
        written, fused = (c - np.float32(lam * three)).astype(np.float32), (c.astype(np.float64) - np.float64(lam) * 3.0).astype(np.float32)
        np.testing.assert_array_equal(hist[:, 3], written)
        told_apart += int((written != fused).any())
    assert told_apart > 0


# ---------------------------------------------------------------- 2. the selection and the scores against float64
def check_run(run, case, variant):
    """the selection (checked when the run was made: check_groups), the ambiguous share, scores and log_probs against float64"""
    b, hid, vocab, layers, w, g = case
    wg = w // g
    fin = np.isfinite(run['hist'])
    err_hist = float(np.abs(run['hist'][fin] - run['fol']['chosen'][fin]).max())
    assert (np.isfinite(run['fol']['chosen']) == fin).all()
    dec, z = run['dec'], run['z']
    plan = torch.from_numpy(run['plan'])
    err_seq = 0.0
    alive = np.isfinite(run['scores'])
    assert (np.isfinite(run['logp']) == alive).all()
    for j in range(w):
        again = dec.score_tokens(z, run['seqs_dev'][:, j].contiguous(), plan=plan).cpu().numpy()
        if alive[:, j].any():
            err_seq = max(err_seq, float(np.abs(again - run['logp'][:, j])[alive[:, j]].max()))
    print(f'diverse beam case {case_id(case)} {variant}: ambiguous selections {run["share"]:.4f}, |scores - float64| {err_hist:.3e}, '
          f'|log_probs - score_tokens| {err_seq:.3e} (bar {SCORE_BAR:.1e})')
    assert run['share'] <= 0.05                                           # beyond that the test proves nothing
    assert err_hist <= SCORE_BAR and err_seq <= SCORE_BAR
    if variant == 'plan':                                                 # per group: min(W', prod |A|) finite slots, dead ones last
        want = finite_counts(run['plan'], wg)
        for i in range(g):
            np.testing.assert_array_equal(fin[..., i * wg:(i + 1) * wg].sum(-1), want)
        rows, ts = np.arange(b)[:, None, None], np.arange(24)[None, None, :]
        assert (run['plan'][rows, ts, run['seqs']] != 0).all()
        assert (run['hist'][~fin] == -np.inf).all() and (wg == 1 or not fin.all())


@pytest.mark.parametrize('case,variant', CASE_VARIANTS, ids=[f'{case_id(c)}_{v}' for c, v in CASE_VARIANTS])
def test_diverse_selection_and_scores_vs_float64(dev, monkeypatch, case, variant):
    check_run(run_of(case, '0', variant, dev, monkeypatch), case, variant)


# ---------------------------------------------------------------- 3. one launch against tick by tick
TWO_LAYER_VARIANTS = [(c, v) for c, v in CASE_VARIANTS if c in TWO_LAYER]


@pytest.mark.parametrize('case,variant', TWO_LAYER_VARIANTS, ids=[f'{case_id(c)}_{v}' for c, v in TWO_LAYER_VARIANTS])
def test_tick_by_tick_path_selects_the_same_groups(dev, monkeypatch, case, variant):
    """ARVAE_TICK_STEPWISE=1 (arvae_beam_select_groups per tick) passes check 2 as well, and codes without an ambiguous selection on
    either path carry identical histories on both"""
    assert one_launch(case)
    step = run_of(case, '1', variant, dev, monkeypatch)
    check_run(step, case, variant)
    np.testing.assert_array_equal(backtrack(step['parents'], step['tokens']), step['seqs'])
    fast = run_of(case, '0', variant, dev, monkeypatch)
    both = clear_prefix(fast['ordered']) & clear_prefix(step['ordered'])     # (B, T): per code the ticks clear so far on both paths
    codes_clear = fast['ordered'].all((1, 2)) & step['ordered'].all((1, 2))
    print(f'diverse beam case {case_id(case)} {variant}: codes clear on both paths {codes_clear.mean():.3f}, ticks {both.mean():.3f}')
    assert both.mean() > 0.3
    fin = np.isfinite(fast['hist'])
    np.testing.assert_array_equal(fin[both], np.isfinite(step['hist'])[both])
    np.testing.assert_array_equal(fast['parents'][both][fin[both]], step['parents'][both][fin[both]])
    np.testing.assert_array_equal(fast['tokens'][both][fin[both]], step['tokens'][both][fin[both]])
    assert np.abs(fast['hist'][both][fin[both]] - step['hist'][both][fin[both]]).max() <= SCORE_BAR


# ---------------------------------------------------------------- 4. end to end
def test_trainer_writes_alternatives(dev):
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    torch.manual_seed(0)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.5, 16, 2, 64, 0.5, False, 'folk')
    trainer = MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))
    trainer.cuda()
    model.eval()
    pads = [ds.note2index_dicts[s] for s in ('START', 'END', None)]
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
        model.decoder.tick_emb_to_note_emb[0].bias[pads] += 3.0            # the padding symbols are the likeliest notes
    score = syn.measure_batch(12, seed=3)
    keep = np.zeros(24, bool)
    keep[:6] = keep[12:18] = True
    seqs, logp = trainer.infill_alternatives(score, keep=keep, playable=True, beam_width=4, beam_groups=2, diversity=0.5)
    assert seqs.shape == (12, 4, 24) and seqs.dtype == torch.int64 and logp.shape == (12, 4) and logp.dtype == torch.float32
    got = seqs.cpu().numpy()
    for j in range(4):
        np.testing.assert_array_equal(got[:, j][:, keep], score[:, keep])  # the kept ticks are the original's in every alternative
        assert not np.isin(got[:, j][:, ~keep], pads).any()
    assert any(not np.array_equal(got[c, 0], got[c, 2]) for c in range(12))    # the groups do write different measures
    plan = trainer.build_note_plan(score, keep=keep, playable=True)
    z = model.encoder.encode_params(torch.from_numpy(score).to(dev).long())[0]
    assert bool(torch.isfinite(logp).all())
    for j in range(4):
        again = model.decoder.score_tokens(z, seqs[:, j].contiguous(), plan=plan)
        assert float((again - logp[:, j]).abs().max()) <= SCORE_BAR
    z = torch.randn(12, 16).to(dev)
    free, _ = trainer.decode_alternatives(z, 4, 2, 0.5)
    assert any(bool((free == p).any()) for p in pads)
    notes, lp = trainer.decode_alternatives(z, 4, 2, 0.5, playable=True)
    assert notes.shape == (12, 4, 24) and int(notes.min()) >= 0 and int(notes.max()) < 35 and lp.shape == (12, 4)
    assert not any(bool((notes == p).any()) for p in pads)
    assert not model.training and model.decoder.sampling == 'argmax' and model.decoder.use_teacher_forcing is True


def test_cli_alternatives_flags(dev, tmp_path):
    """--test --sample 3 --infill 2 --keep_ticks 0-5 --beam 4 --beam_groups 2 --diversity 0.5 on a model saved by a one-epoch synthetic
    run prints three prior draws' and two measures' four alternatives, the kept ticks the original's in each of the latter"""
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    common = ['--batch_size', '16', '--rand', '1', '-r', 'all', '--encoder_hidden_size', '64', '--decoder_hidden_size', '64']
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(tmp_path / 'models'))
    flags = ['--sample', '3', '--infill', '2', '--keep_ticks', '0-5', '--beam', '4', '--beam_groups', '2', '--diversity', '0.5']
    for extra in (['--num_epochs', '1'], ['--test'] + flags):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + extra + common, capture_output=True, text=True,
                           timeout=600, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]
    assert summary['sampling'] == {'beam': 4, 'beam_groups': 2, 'diversity': 0.5, 'playable': False}
    assert len(summary['samples']) == len(summary['alternatives']) == 3
    for first, alt in zip(summary['samples'], summary['alternatives']):
        assert len(alt['measures']) == 4 == len(alt['log_probs']) and alt['measures'][0] == first
        assert all(len(m) == 24 and set(m) <= set(n2i) for m in alt['measures']) and all(x <= 0 for x in alt['log_probs'])
    infill = summary['infill']
    assert infill['sampling'] == 'beam' and infill['beam_groups'] == 2 and infill['diversity'] == 0.5
    assert len(infill['original']) == len(infill['infilled']) == len(infill['alternatives']) == 2
    for old, new, alt in zip(infill['original'], infill['infilled'], infill['alternatives']):
        assert len(alt['measures']) == 4 == len(alt['log_probs']) and alt['measures'][0] == new
        assert all(isinstance(x, float) and x <= 0 for x in alt['log_probs'])
        for m in alt['measures']:
            assert len(m) == 24 and set(m) <= set(n2i) and m[:6] == old[:6]

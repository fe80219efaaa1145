"""Beam search of the MeasureVAE decoder on the device (include/arvae_hip.h, "Beam search"): exact properties of the histories, the
selection step by step against the float64 follower of tests/test_beam_search.py, the scores against a measured bar, the row kernel
sequence_log_prob against float64, the one-launch kernel against the tick-by-tick path, the trainer's surface and the command line."""
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
import layer_stack_ref as ref  # noqa: E402
from test_beam_search import (CASES, DELTA, OTHER_SHAPES, Stepper64, backtrack, case_id, check_history, codes, follow64, half_mask, logp64,  # noqa: E402
                              make_decoder, params64)
from test_sampling import _FolkDataset  # noqa: E402

# The bar of the score checks, measured and not guessed (`weight_path_error` below, run over CASES on an MI355X, one launch and tick by
# tick alike).  The code
# paths of the parent commit -- generate(z, 'argmax'): the free-running kernels' tokens, the whole-sequence kernels' weights -- against
# float64 weights on the same tokens: the largest per-measure |sum_t logp(w_device) - sum_t logp(w_float64)| was
SCORE_ERR_MEASURED = 7.5629e-06        # (case b600_h64_v35_l2_w4; the others 2.1e-06 .. 6.6e-06; OTHER_SHAPES' 9.9e-07, 2.8e-06)
# and the bar is four times that: the margin covers the beam kernel's own log-softmax and its 24-term running fp32 sum
SCORE_BAR = 4.0 * SCORE_ERR_MEASURED   # 3.0252e-05; 2 x bar = 6.1e-05 <= DELTA = 1e-3
TWO_LAYER = [c for c in CASES if c[3] == 2]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def weight_path_error(case, dev):
    """the largest per-measure |sum_t logp(w_device)[tok] - sum_t logp(w_float64 on the same tokens)[tok]| of generate(z, 'argmax')"""
    b, hid, vocab, layers, _ = case
    dec = make_decoder(hid, vocab, layers).cuda()
    z = codes(b)
    weights, samples = dec.generate(torch.from_numpy(z).to(dev), sampling='argmax')
    tok = samples[:, 0].cpu()
    w64 = ref.decode(params64(dec), torch.from_numpy(z).double(), tok, True)[0].numpy()
    pick = lambda w: np.take_along_axis(logp64(w), tok.numpy()[..., None], -1)[..., 0].sum(-1)
    return float(np.abs(pick(weights.double().cpu().numpy()) - pick(w64)).max())


def test_the_score_bar_leaves_the_margin_clear():
    assert 2.0 * SCORE_BAR <= DELTA


_RUNS = {}


def beam_run(case, mode, masked, dev, monkeypatch):
    """one beam search of a case with ARVAE_TICK_STEPWISE = mode, and its float64 follower, once"""
    key = (case, mode, masked)
    if key not in _RUNS:
        b, hid, vocab, layers, w = case
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        dec = make_decoder(hid, vocab, layers).cuda()
        z = torch.from_numpy(codes(b)).to(dev)
        allow = half_mask(vocab) if masked else None
        weights, samples, best, seqs, scores, (parents, tokens, hist) = dec.beam_search(z, w, allowed=allow, return_history=True)
        assert dec.training and dec.use_teacher_forcing is True and dec.sampling == 'argmax' and dec._filter is None
        assert weights.shape == (b, 24, vocab) and samples.shape == (b, 1, 24) and samples.dtype == torch.int64 and best.shape == (b,)
        assert seqs.shape == (b, w, 24) and seqs.dtype == torch.int64 and scores.shape == (b, w) and scores.dtype == torch.float32
        assert parents.shape == tokens.shape == hist.shape == (b, 24, w)
        assert parents.dtype == torch.int32 and tokens.dtype == torch.int64 and hist.dtype == torch.float32
        run = dict(dec=dec, z=z, allow=allow, weights=weights, samples=samples[:, 0].cpu().numpy(), best=best.cpu().numpy(),
                   seqs=seqs.cpu().numpy(), scores=scores.cpu().numpy(), parents=parents.cpu().numpy(), tokens=tokens.cpu().numpy(),
                   hist=hist.cpu().numpy(), seqs_dev=seqs)
        run['fol'] = follow64(Stepper64(params64(dec), codes(b), w), run['parents'], run['tokens'], w, allow)
        _RUNS[key] = run
    return _RUNS[key]


def one_launch(case):
    return case[3] == 2 and ops.tick_beam_search_supported(case[1], case[2], case[4])


def maskable(case):
    return case[4] <= int(half_mask(case[2]).sum())


# ---------------------------------------------------------------- 1. exact, oracle-free
@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_beam_histories_exact_properties(dev, monkeypatch, case):
    b, hid, vocab, layers, w = case
    assert one_launch(case) == (layers == 2)
    run = beam_run(case, '0', False, dev, monkeypatch)
    dec, z = run['dec'], run['z']
    # the history backtracks to the sequences; the best beam is what the call returns first
    np.testing.assert_array_equal(backtrack(run['parents'], run['tokens']), run['seqs'])
    np.testing.assert_array_equal(run['samples'], run['seqs'][:, 0])
    np.testing.assert_array_equal(run['best'], run['scores'][:, 0])
    np.testing.assert_array_equal(run['scores'], run['hist'][:, -1])
    assert run['tokens'].min() >= 0 and run['tokens'].max() < vocab and run['parents'].min() >= 0 and run['parents'].max() < w
    assert (run['parents'][:, 0] == 0).all()                              # tick 0: one live beam
    # distinct, non-increasing, finite
    assert np.isfinite(run['hist']).all() and (np.diff(run['hist'], axis=-1) <= 0).all()
    for code in range(b):
        assert len({tuple(s) for s in run['seqs'][code]}) == w, code
    # a beam of one is the argmax free run, bit for bit (shapes without a one-launch kernel: both tick by tick)
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', '0' if layers == 2 else '1')
    greedy = dec.generate(z, sampling='argmax')[1]
    one = dec.beam_search(z, beam_width=1)
    assert torch.equal(one[1], greedy) and one[3].shape == (b, 1, 24)
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', '0')
    # beams of a ragged tail never leak into live codes: the same codes in a batch that fills the tiles (other codes behind them);
    # codes without an ambiguous step carry the same history, and every code's scores agree within the bar
    full = -(-b // 16) * 16 + 16
    zf = torch.cat((z, torch.from_numpy(syn.normal_noise((full - b, 32), seed=31)).to(dev)), 0)
    filled = dec.beam_search(zf, w, return_history=True)
    _, clear = check_history(run['fol'], run['parents'], run['tokens'], w)
    rows = clear.all(1)
    assert rows.any()
    np.testing.assert_array_equal(filled[5][0][:b].cpu().numpy()[rows], run['parents'][rows])
    np.testing.assert_array_equal(filled[5][1][:b].cpu().numpy()[rows], run['tokens'][rows])
    assert np.abs(filled[4][:b].cpu().numpy()[rows] - run['scores'][rows]).max() <= SCORE_BAR
    # a random half mask, note 0 banned: no banned note in any beam at any tick
    if maskable(case):
        masked = beam_run(case, '0', True, dev, monkeypatch)
        assert masked['allow'][masked['tokens']].all() and masked['allow'][masked['seqs']].all()
        assert np.isfinite(masked['hist']).all() and len(np.unique(masked['tokens'])) > 3
    # a mask of W notes: tick 0's beams are exactly those notes, in logp order (the order of tick 0's weights where they stand clear)
    few = np.zeros(vocab, np.uint8)
    few[np.random.RandomState(11).permutation(vocab)[:w]] = 1
    res = dec.beam_search(z, w, allowed=few, return_history=True)
    first = res[5][1][:, 0].cpu().numpy()
    w0 = res[0][:, 0].double().cpu().numpy()
    notes = np.flatnonzero(few)
    for code in range(b):
        assert sorted(first[code]) == list(notes), code
        order = notes[np.argsort(-w0[code, notes], kind='stable')]
        gaps = -np.diff(w0[code, order])
        if (gaps > DELTA).all():
            np.testing.assert_array_equal(first[code], order)
    assert few[res[5][1].cpu().numpy()].all()


# ---------------------------------------------------------------- 2. / 3. the selection and the scores against float64
def check_run(run, case, dev):
    """checks 2 and 3 of a run -> the clear steps (B, T)"""
    w = case[4]
    share, clear = check_history(run['fol'], run['parents'], run['tokens'], w)
    err_hist = float(np.abs(run['hist'] - run['fol']['chosen']).max())
    dec, z, allow = run['dec'], run['z'], run['allow']
    err_seq = 0.0
    for j in range(w):
        again = dec.score_tokens(z, run['seqs_dev'][:, j].contiguous(), allowed=allow).cpu().numpy()
        err_seq = max(err_seq, float(np.abs(again - run['scores'][:, j]).max()))
    print(f'beam case {case_id(case)} mask {allow is not None}: ambiguous steps {share:.4f}, |scores - float64| {err_hist:.3e}, '
          f'|scores - score_tokens| {err_seq:.3e} (bar {SCORE_BAR:.1e})')
    assert share <= 0.05                                                  # beyond that the test proves nothing
    assert err_hist <= SCORE_BAR and err_seq <= SCORE_BAR
    return clear


@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_beam_selection_and_scores_vs_float64(dev, monkeypatch, case):
    check_run(beam_run(case, '0', False, dev, monkeypatch), case, dev)
    if maskable(case):
        check_run(beam_run(case, '0', True, dev, monkeypatch), case, dev)


@pytest.mark.parametrize('case', OTHER_SHAPES, ids=[case_id(c) for c in OTHER_SHAPES])
def test_shapes_without_a_one_launch_kernel_search_tick_by_tick(dev, monkeypatch, case):
    assert not ops.tick_beam_search_supported(case[1], case[2], case[4])
    run = beam_run(case, '0', False, dev, monkeypatch)
    np.testing.assert_array_equal(backtrack(run['parents'], run['tokens']), run['seqs'])
    check_run(run, case, dev)
    check_run(beam_run(case, '0', True, dev, monkeypatch), case, dev)


# ---------------------------------------------------------------- 4. sequence_log_prob against float64 on given logits
@pytest.mark.parametrize('vocab', (1, 16, 35, 64, 200))
def test_sequence_log_prob_vs_float64(dev, vocab):
    """257 rows of 24 ticks of relu(N(0, 2)) logits (exact inputs), with and without a mask that keeps half the notes: the absolute
    error is at most 24 * 16 * 2^-24 * max(1, max|l| + ln V), 16 ulp per tick at the largest magnitude involved"""
    rs = np.random.RandomState(100 + vocab)
    logits = np.maximum(rs.normal(size=(257, 24, vocab)) * 2.0, 0.0).astype(np.float32)
    bound = 24 * 16 * 2.0 ** -24 * max(1.0, float(np.abs(logits).max()) + np.log(vocab))
    for masked in (False, True):
        allow = None
        if masked:
            allow = np.zeros(vocab, np.uint8)
            allow[rs.permutation(vocab)[:max(1, vocab // 2)]] = 1
        notes = np.arange(vocab) if allow is None else np.flatnonzero(allow)
        tok = notes[rs.randint(0, len(notes), size=(257, 24))]
        got = ops.sequence_log_prob(torch.from_numpy(logits).to(dev), torch.from_numpy(tok).to(dev),
                                    None if allow is None else torch.from_numpy(allow).to(dev))
        assert got.shape == (257,) and got.dtype == torch.float32
        want = np.take_along_axis(logp64(logits, allow), tok[..., None], -1)[..., 0].sum(-1)
        err = float(np.abs(got.double().cpu().numpy() - want).max())
        print(f'sequence_log_prob vocab {vocab} mask {masked}: max error {err:.3e}, bound {bound:.3e}')
        assert err <= bound
        if masked and vocab > 1:                                          # a banned token has no probability
            bad = tok.copy()
            bad[0, 3] = np.flatnonzero(allow == 0)[0]
            got = ops.sequence_log_prob(torch.from_numpy(logits).to(dev), torch.from_numpy(bad).to(dev), torch.from_numpy(allow).to(dev))
            assert float(got[0]) == -np.inf and bool(torch.isfinite(got[1:]).all())


# ---------------------------------------------------------------- 5. one launch against tick by tick
@pytest.mark.parametrize('case', TWO_LAYER, ids=[case_id(c) for c in TWO_LAYER])
def test_tick_by_tick_path_selects_the_same_beams(dev, monkeypatch, case):
    """ARVAE_TICK_STEPWISE=1 (the dense and gate launches and arvae_beam_select per tick) passes checks 2 and 3 as well, and codes
    without an ambiguous step on either path carry identical histories on both"""
    assert one_launch(case)
    step = beam_run(case, '1', False, dev, monkeypatch)
    clear1 = check_run(step, case, dev)
    np.testing.assert_array_equal(backtrack(step['parents'], step['tokens']), step['seqs'])
    fast = beam_run(case, '0', False, dev, monkeypatch)
    _, clear0 = check_history(fast['fol'], fast['parents'], fast['tokens'], case[4])
    both = clear0.all(1) & clear1.all(1)
    assert both.mean() > 0.3
    np.testing.assert_array_equal(fast['parents'][both], step['parents'][both])
    np.testing.assert_array_equal(fast['tokens'][both], step['tokens'][both])
    assert np.abs(fast['hist'][both] - step['hist'][both]).max() <= SCORE_BAR


# ---------------------------------------------------------------- 6. end to end
def test_trainer_decodes_playable_measures_by_beam_search(dev):
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
    z = torch.randn(12, 16).to(dev)
    _, free = trainer.decode_latent_codes(z, sampling='beam', beam_width=4)
    assert any(bool((free == p).any()) for p in pads)
    _, notes = trainer.decode_latent_codes(z, sampling='beam', beam_width=4, playable=True)
    assert notes.shape == (12, 1, 24) and notes.dtype == torch.int64 and int(notes.min()) >= 0 and int(notes.max()) < 35
    assert not any(bool((notes == p).any()) for p in pads)
    wide = model.decoder.beam_search(z, beam_width=4, allowed=trainer.playable_mask())
    assert torch.equal(wide[1], notes) and bool(torch.isfinite(wide[4]).all())
    _, drawn = trainer.sample_measures(8, playable=True, beam_width=4)
    assert drawn.shape == (8, 1, 24) and not any(bool((drawn == p).any()) for p in pads)
    assert not model.training and model.decoder.sampling == 'argmax' and model.decoder.use_teacher_forcing is True


def test_cli_beam_flag(dev, tmp_path):
    """--sample 8 --beam 4 --playable on a two-epoch synthetic run prints eight measures of 24 names, none a padding symbol"""
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    args = ['--num_epochs', '2', '--sample', '8', '--beam', '4', '--playable', '--batch_size', '16', '--rand', '1', '-r', 'all',
            '--encoder_hidden_size', '64', '--decoder_hidden_size', '64']
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(tmp_path / 'models'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + args, capture_output=True, text=True, timeout=600,
                       env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]
    assert summary['sampling'] == {'beam': 4, 'playable': True}
    assert len(summary['samples']) == 8 and all(len(m) == 24 for m in summary['samples'])
    names = {s for m in summary['samples'] for s in m}
    assert names <= set(n2i) and not names & {'START', 'END', None, 'None'}

"""Top-k, nucleus (top-p) and note-mask sampling of the free-running decoder on the device (include/arvae_hip.h,
arvae_sample_filter_t): the row sampler against the float64 restatement of tests/test_sampling_filters.py, exact properties of the
one-launch kernels' PICK_FILTERED, their picks against the weights the whole-sequence kernels return, the tick-by-tick path, the
trainer's `playable` mask and the command line."""
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
from oracle import philox

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampling import _FolkDataset  # noqa: E402
from test_sampling_filters import (DELTA_ROW, ROW_COLS, ROW_PARAMS, check_row_picks, check_tick_picks, filter64,  # noqa: E402
                                   pick64_filtered, row_case)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


# ---------------------------------------------------------------- 1. the row sampler against float64 on given logits
@pytest.mark.parametrize('cols', ROW_COLS)
def test_row_sample_filtered_vs_float64(dev, cols):
    """257 rows of relu(N(0, 2)) logits (exact zeros present), every (top_k, top_p) of ROW_PARAMS with and without a mask that keeps
    half the notes.  The logits are exact inputs, so the ranks are exact: only the top_p boundary and the CDF can differ (band
    DELTA_ROW = 1e-5, test_sampling_gpu's).  Clear draws equal the float64 pick, ambiguous ones lie in the keep-set at top_p + delta."""
    for top_k, top_p, tau in ROW_PARAMS:
        for masked in (False, True):
            logits, u, allow, k = row_case(cols, top_k, top_p, masked)
            tok = ops.row_sample_filtered(torch.from_numpy(logits).to(dev), torch.from_numpy(u).to(dev), tau, top_k=k, top_p=top_p,
                                          allow=None if allow is None else torch.from_numpy(allow).to(dev))
            assert tok.shape == (logits.shape[0],) and tok.dtype == torch.int64
            tok = tok.cpu().numpy()
            share = check_row_picks(tok, logits, u, tau, allow, k, top_p, DELTA_ROW)
            print(f'row_sample_filtered cols {cols} top_k {k} top_p {top_p} mask {masked}: ambiguous draws {share:.5f}')
            assert share <= 0.05
            if allow is not None:
                assert allow[tok].all()
            if k == 1:
                np.testing.assert_array_equal(tok, np.where(allow if allow is not None else np.ones(cols, bool), logits, -1.0).argmax(1))
    with pytest.raises(RuntimeError, match='top_p'):
        ops.row_sample_filtered(torch.zeros(2, cols, device=dev), torch.ones(2, device=dev), 1.0, top_p=1.5)
    with pytest.raises(RuntimeError, match='top_k'):
        ops.row_sample_filtered(torch.zeros(2, cols, device=dev), torch.ones(2, device=dev), 1.0, top_k=cols + 1)


# ---------------------------------------------------------------- the decoders of checks 2 to 4
def _decoder(hid, vocab, layers=2, seed=23):
    """test_sampling_gpu._decoder for any layer count: output weights x 4, bias + 0.3, so that the notes vary"""
    from arvae_amd.measure_vae import HierarchicalDecoder
    torch.manual_seed(seed)
    dec = HierarchicalDecoder(10, vocab, 32, layers, hid, 0.0).cuda().train()
    with torch.no_grad():
        dec.tick_emb_to_note_emb[0].weight.mul_(4.0)
        dec.tick_emb_to_note_emb[0].bias.add_(0.3)
    dec.teacher_forcing_prob = 0.0
    return dec


def _inputs(b, dev, edges=False):
    """latent codes and draws (b, 24) in (0, 1]; edges: every third row draws u = 1 at every tick (the draw the last survivor's own
    prefix has to reach: a total taken from another lane's sum can lie one ulp above it) and row 1 the smallest u, 2^-32"""
    z = torch.from_numpy(syn.normal_noise((b, 32), seed=29)).to(dev)
    u = np.asarray(philox.unit(philox.blocks(b * 24, 1234, 7, 0)[:, 0]), np.float32).reshape(b, 24)
    if edges:
        u[::3] = 1.0
        u[1] = 2.0 ** -32
    return z, u


def _half_mask(vocab):
    allow = np.zeros(vocab, np.uint8)
    allow[np.random.RandomState(7).permutation(vocab)[:vocab // 2]] = 1
    return allow


# ---------------------------------------------------------------- 2. exact properties of the one-launch kernels
# (batch, hidden, vocab, layers): the issue's six, and the 8- and 16-row workgroups of both kernels' other instantiations
EXACT_CASES = [(21, 128, 35, 2),         # ragged batch, 4 rows per workgroup
               (37, 64, 16, 2),          # one logits tile
               (45, 32, 32, 2),          # two tiles
               (64, 128, 64, 2),         # four tiles
               (21, 64, 35, 1),          # the layers kernel, one layer
               (21, 64, 35, 3),          # the layers kernel, three layers
               (1501, 128, 35, 2),       # 8 rows per workgroup
               (2101, 64, 35, 2),        # 16 rows per workgroup
               (1501, 64, 35, 1)]        # the layers kernel at 8 rows per workgroup


@pytest.mark.parametrize('case', EXACT_CASES, ids=[f'b{c[0]}_h{c[1]}_v{c[2]}_l{c[3]}' for c in EXACT_CASES])
def test_filtered_kernel_exact_properties(dev, monkeypatch, case):
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', '0')
    b, hid, vocab, layers = case
    assert ops.tick_free_run_supported(hid, vocab) if layers == 2 else ops.tick_free_run_layers_supported(hid, vocab, layers)
    dec = _decoder(hid, vocab, layers)
    z, u = _inputs(b, dev, edges=True)
    ut = torch.from_numpy(u)
    greedy = dec.generate(z, sampling='argmax')[1]
    plain = dec.generate(z, uniforms=ut, temperature=0.8)[1]
    assert greedy.shape == plain.shape == (b, 1, 24) and not torch.equal(greedy, plain)
    # top_k = 1 is the argmax free run, bit for bit, whatever the other cut and the temperature
    assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, top_k=1)[1], greedy)
    assert torch.equal(dec.generate(z, uniforms=ut, temperature=1.7, top_k=1, top_p=0.5)[1], greedy)
    # no filter active: the unfiltered draw, bit for bit
    for kw in ({'top_k': vocab}, {'top_p': 1.0}, {'top_k': vocab, 'top_p': 1.0}):
        assert torch.equal(dec.generate(z, uniforms=ut, temperature=0.8, **kw)[1], plain), kw
    # a mask of one note gives that note at every tick
    for note in (0, vocab // 2, vocab - 1):
        one = np.zeros(vocab, np.uint8)
        one[note] = 1
        got = dec.generate(z, uniforms=ut, temperature=0.8, allowed=one, top_p=0.9)[1]
        assert got.shape == (b, 1, 24) and bool((got == note).all()), note
    # a random mask: no banned note is ever emitted, alone and under both cuts, at several temperatures (a third of the rows
    # draw u = 1 throughout: some 500 to 17000 such draws per call); note 0, what an empty search would return, is banned
    allow = _half_mask(vocab)
    allow[0] = 0
    for tau in (0.8, 0.7, 1.3):
        for kw in ({}, {'top_k': 3}, {'top_p': 0.7}, {'top_k': 5, 'top_p': 0.8}):
            got = dec.generate(z, uniforms=ut, temperature=tau, allowed=allow, **kw)[1].cpu().numpy()
            assert got.min() >= 0 and got.max() < vocab and allow[got].all(), (tau, kw, np.unique(got[~allow[got].astype(bool)]))
            assert len(np.unique(got)) > 1
    # the cuts bite: with top_k = 2 a tick's note is one of the two largest returned weights wherever those stand clear; the rows
    # that draw u = 1 take the one with the higher index (the last survivor), the row that draws 2^-32 the one with the lower
    w, got = dec.generate(z, uniforms=ut, temperature=0.8, top_k=2)
    top3 = torch.topk(w, 3, dim=2)
    clear = (top3.values[..., 1] - top3.values[..., 2]) > 1e-3
    pair, got = top3.indices[..., :2], got[:, 0]
    assert bool((got[..., None] == pair).any(-1)[clear].all()) and float(clear.float().mean()) > 0.5
    assert torch.equal(got[::3][clear[::3]], pair.max(-1).values[::3][clear[::3]])
    assert torch.equal(got[1][clear[1]], pair.min(-1).values[1][clear[1]])
    assert dec.training and dec.sampling == 'argmax' and dec._filter is None


# ---------------------------------------------------------------- 3. / 4. picks against the returned weights, both paths
# (batch, hidden, vocab, layers, top_k, top_p, tau, masked).  The cuts fall among well-separated live notes (the dead tail's
# mass_before values are dense near 1): fixed from a CPU run of tests/layer_stack_ref.py on these decoders, float64 weights of the
# argmax trajectory against the picks of a copy rounded to float32 -- that copy passed check_tick_picks everywhere, and the float64
# side's own ambiguous shares were (unmasked / masked)
FILTER_CASES = [(21, 128, 35, 2, 4, 0.8, 0.6, False),     # 0.0000 / 0.0020
                (37, 64, 16, 2, 3, 0.7, 0.5, True),       # 0.0023 / 0.0000
                (45, 32, 32, 2, 5, 0.8, 0.7, False),      # 0.0019 / 0.0046
                (64, 128, 64, 2, 3, 0.6, 0.5, True),      # 0.0026 / 0.0020
                (21, 64, 35, 1, 3, 0.7, 0.5, False),      # 0.0020 / 0.0060
                (21, 64, 35, 3, 4, 0.8, 0.6, True)]       # 0.0000 / 0.0060
# always tick by tick: hidden 128 with three layers, vocabulary 35 at hidden 32
STEPWISE_ONLY = [(21, 128, 35, 3, 4, 0.8, 0.6, False),    # 0.0040 / 0.0000
                 (21, 32, 35, 2, 5, 0.8, 0.7, True)]      # 0.0000 / 0.0020
_RUNS = {}


def _id(c):
    return f'b{c[0]}_h{c[1]}_v{c[2]}_l{c[3]}_k{c[4]}_p{c[5]}_t{c[6]}_m{int(c[7])}'


def filtered_run(case, mode, dev, monkeypatch):
    """(tokens (b, 24), clear rows) of a case with ARVAE_TICK_STEPWISE = mode, once: every emitted note is the float64 filtered pick
    from the returned weights (band: eps = 1e-5 max|w| + 1e-6, delta = 2 eps / tau + 1e-5), the ambiguous share <= 0.05"""
    if (case, mode) not in _RUNS:
        b, hid, vocab, layers, top_k, top_p, tau, masked = case
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        dec = _decoder(hid, vocab, layers)
        z, u = _inputs(b, dev)
        allow = _half_mask(vocab) if masked else None
        before = ops.RngState.offset
        weights, samples = dec.generate(z, temperature=tau, uniforms=torch.from_numpy(u), top_k=top_k, top_p=top_p, allowed=allow)
        assert ops.RngState.offset == before                              # every draw was an explicit input
        assert samples.shape == (b, 1, 24) and samples.dtype == torch.int64 and weights.shape == (b, 24, vocab)
        tok = samples[:, 0].cpu().numpy()
        w = weights.double().cpu().numpy()
        eps = 1e-5 * float(np.abs(w).max()) + 1e-6
        delta = 2.0 * eps / tau + 1e-5
        share, clear = check_tick_picks(tok, w, u, tau, allow, top_k, top_p, eps, delta)
        print(f'filtered case {_id(case)} stepwise {mode}: delta {delta:.3e}, ambiguous draws {share:.5f}, distinct notes {len(np.unique(tok))}')
        assert share <= 0.05                                              # beyond that the test proves nothing
        assert len(np.unique(tok)) > 3
        kept = filter64(w, allow, top_k, top_p, tau).sum(-1)
        assert kept.max() <= top_k and kept.min() >= 1 and kept.mean() < top_k     # the nucleus cut is active as well
        _RUNS[(case, mode)] = (tok, clear.all(1))
    return _RUNS[(case, mode)]


@pytest.mark.parametrize('case', FILTER_CASES, ids=[_id(c) for c in FILTER_CASES])
def test_filtered_kernel_samples_its_own_weights(dev, monkeypatch, case):
    filtered_run(case, '0', dev, monkeypatch)


@pytest.mark.parametrize('case', FILTER_CASES, ids=[_id(c) for c in FILTER_CASES])
def test_per_tick_path_filters_the_same_notes(dev, monkeypatch, case):
    """ARVAE_TICK_STEPWISE=1 (arvae_row_sample_filtered per tick) passes the same check, and rows without an ambiguous draw in either
    mode carry identical notes in both"""
    tok1, clear1 = filtered_run(case, '1', dev, monkeypatch)
    tok0, clear0 = filtered_run(case, '0', dev, monkeypatch)
    both = clear0 & clear1
    assert both.mean() > 0.5
    np.testing.assert_array_equal(tok0[both], tok1[both])


@pytest.mark.parametrize('case', STEPWISE_ONLY, ids=[_id(c) for c in STEPWISE_ONLY])
def test_shapes_without_a_one_launch_kernel_filter_tick_by_tick(dev, monkeypatch, case):
    _, hid, vocab, layers = case[:4]
    assert not (ops.tick_free_run_supported(hid, vocab) if layers == 2 else ops.tick_free_run_layers_supported(hid, vocab, layers))
    filtered_run(case, '0', dev, monkeypatch)


# ---------------------------------------------------------------- the trainer's surface
def test_playable_measures_hold_no_padding_symbol(dev):
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
    ops.rng_reseed(21)
    _, free = trainer.sample_measures(64, temperature=0.9)
    assert any(bool((free == p).any()) for p in pads)
    ops.rng_reseed(21)
    _, notes = trainer.sample_measures(64, temperature=0.9, playable=True)
    assert notes.shape == (64, 1, 24) and notes.dtype == torch.int64 and int(notes.min()) >= 0 and int(notes.max()) < 35
    assert not any(bool((notes == p).any()) for p in pads) and len(torch.unique(notes)) > 3
    _, cut = trainer.sample_measures(64, temperature=0.9, top_k=4, top_p=0.9, playable=True)
    assert not any(bool((cut == p).any()) for p in pads)
    z = torch.randn(6, 16).to(dev)
    u = torch.from_numpy(np.asarray(philox.unit(philox.blocks(6 * 24, 3, 0, 0)[:, 0]), np.float32).reshape(6, 24))
    only = np.zeros(35, np.uint8)
    only[[pads[0], 7, 20]] = 1
    _, a = trainer.decode_latent_codes(z, sampling='multinomial', temperature=1.5, uniforms=u, allowed=only, playable=True)
    _, b = trainer.decode_latent_codes(z, sampling='multinomial', temperature=1.5, uniforms=u, allowed=only, playable=True)
    assert torch.equal(a, b) and set(torch.unique(a).tolist()) <= {7, 20}
    assert not model.training and model.decoder.sampling == 'argmax' and model.decoder._filter is None


# ---------------------------------------------------------------- 5. the command line
def _run_cli(args, env_dir):
    env = dict(os.environ, ARVAE_DATA_DIR=str(env_dir), ARVAE_MODEL_DIR=str(env_dir / 'models'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + args, capture_output=True, text=True, timeout=600,
                       env=env, cwd=str(env_dir))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]


def test_cli_filter_flags(dev, tmp_path):
    """--sample 8 --top_k 4 --top_p 0.9 --playable on a two-epoch synthetic run prints eight measures of 24 names, none a padding
    symbol, and echoes the flags"""
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    common = ['--batch_size', '16', '--rand', '1', '-r', 'all', '--encoder_hidden_size', '64', '--decoder_hidden_size', '64']
    summary = _run_cli(['--num_epochs', '2', '--sample', '8', '--top_k', '4', '--top_p', '0.9', '--playable'] + common, tmp_path)
    assert summary['sampling'] == {'temperature': 1.0, 'top_k': 4, 'top_p': 0.9, 'playable': True}
    assert len(summary['samples']) == 8 and all(len(m) == 24 for m in summary['samples'])
    names = {s for m in summary['samples'] for s in m}
    assert names <= set(n2i) and not names & {'START', 'END', None, 'None'}

"""Multinomial feedback of the hierarchical decoder on the device (measurevae/decoder.py:372,431-434,502-505;
measure_vae.py:133-166): the library's uniforms, the row sampler and the one-launch tick kernel's pick stage against the float64
picker of tests/test_sampling.py, the two decoder paths against each other, a training step, forward_test, the trainer's and the
command line's surface."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arvae_amd  # noqa: F401
from arvae_amd import _lib, ops
from arvae_amd import synthetic as syn
from oracle import philox

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sampling import _FolkDataset, cdf64, check_picks, chi_square, pick64  # noqa: E402

# 99.9 % points of the chi-square distribution, degrees of freedom 1 .. 40
CHI2_999 = [10.828, 13.816, 16.266, 18.467, 20.515, 22.458, 24.322, 26.124, 27.877, 29.588, 31.264, 32.909, 34.528, 36.123, 37.697,
            39.252, 40.790, 42.312, 43.820, 45.315, 46.797, 48.268, 49.728, 51.179, 52.620, 54.052, 55.476, 56.892, 58.301, 59.703,
            61.098, 62.487, 63.870, 65.247, 66.619, 67.985, 69.346, 70.703, 72.055, 73.402]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def library_uniforms(n, seed, offset, dev):
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().arvae_philox_uniform(ctypes.c_void_p(out.data_ptr()), n, seed, offset, 0, None,
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'philox_uniform')
    return out


# ---------------------------------------------------------------- 1. uniforms
def test_philox_uniform_vs_oracle(dev):
    got = library_uniforms(1000, 77, 3, dev).cpu().numpy()
    want = philox.unit(philox.blocks(1000, 77, 3, 0)[:, 0])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
    assert got.min() > 0.0 and got.max() <= 1.0
    torch.manual_seed(5)
    ops.rng_reseed(5)
    a = ops.philox_uniform((3, 24), dev)
    b = ops.philox_uniform((3, 24), dev)                                   # the next offset of the step: another draw
    assert a.shape == (3, 24) and not torch.equal(a, b) and ops.RngState.offset == 2
    np.testing.assert_array_equal(a.cpu().numpy().ravel(), np.asarray(philox.unit(philox.blocks(72, ops.rng_seed(), 0, 0)[:, 0]), np.float32))


# ---------------------------------------------------------------- 2. the row sampler against float64
DELTA_ROW = 1e-5          # 130 fp32 additions at 2^-24 relative each (8e-6) + the exponential's ulps


@pytest.mark.parametrize('tau', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('cols', [1, 16, 35, 64, 130])
def test_row_sample_vs_float64(dev, cols, tau):
    rs = np.random.RandomState(100 * cols + int(10 * tau))
    rows = 777
    logits = np.maximum(rs.normal(size=(rows, cols)) * 2.0 + 0.3, 0.0).astype(np.float32)
    u = (1.0 - rs.random_sample(rows)).astype(np.float32)               # (0, 1]
    u = np.clip(u, np.float32(2.0 ** -32), np.float32(1.0))
    u[:2] = [1.0, 2.0 ** -32]                                            # the ends of the range on ordinary rows
    # edge rows: all-zero logits (the uniform distribution) and one logit of 1e4 among zeros, each at the range's ends and inside
    edge_u = np.array([1.0, 2.0 ** -32, 0.5, (cols // 3 + 0.5) / cols], np.float32)
    hot = cols // 2
    logits[2:6] = 0.0
    u[2:6] = edge_u
    logits[6:10] = 0.0
    logits[6:10, hot] = 1e4
    u[6:10] = edge_u
    tok = ops.row_sample(torch.from_numpy(logits).to(dev), torch.from_numpy(u).to(dev), tau)
    assert tok.shape == (rows,) and tok.dtype == torch.int64
    tok = tok.cpu().numpy()
    band = check_picks(tok, logits, u, tau, DELTA_ROW)
    print(f'row_sample cols {cols} tau {tau}: band draws {band:.5f}')
    assert band <= 0.05
    assert tok[1] == 0
    np.testing.assert_array_equal(tok[2:6], np.ceil(edge_u.astype(np.float64) * cols).astype(np.int64) - 1)
    np.testing.assert_array_equal(tok[6:10], hot)
    if cols == 1:
        assert not tok.any()
    with pytest.raises(RuntimeError, match='inverse temperature'):
        ops.row_sample(torch.from_numpy(logits).to(dev), torch.from_numpy(u).to(dev), float('nan'))


# ---------------------------------------------------------------- 3. the distribution
DIST_LOGITS = np.maximum(np.random.RandomState(5).normal(size=35) * 2.0 + 0.3, 0.0)


@pytest.mark.parametrize('tau,critical,bins', [(1.0, 65.2, 35), (2.0, 65.2, 35), (0.5, 31.3, 12)])
def test_row_sample_distribution(dev, tau, critical, bins):
    """65536 draws of one row: chi-square below the 99.9 % point (34 / 34 / 11 degrees of freedom); the float64 picker on these
    uniforms gives 22.3, 20.6 and 12.8, and the draws are a pure function of (seed, offset): nothing here can flake"""
    n = 65536
    u = library_uniforms(n, 77, 3, dev)
    logits = torch.from_numpy(DIST_LOGITS.astype(np.float32)).to(dev)[None].expand(n, -1).contiguous()
    tok = ops.row_sample(logits, u, tau).cpu().numpy()
    chi, kept = chi_square(tok, DIST_LOGITS.astype(np.float32), tau)
    ref, _ = chi_square(pick64(np.broadcast_to(DIST_LOGITS.astype(np.float32), (n, 35)), u.cpu().numpy(), tau)[0], DIST_LOGITS.astype(np.float32), tau)
    print(f'row_sample distribution tau {tau}: chi-square {chi:.2f} over {kept} bins (float64 picker {ref:.2f}), critical {critical}')
    assert kept == bins and chi < critical


def _decoder(hid, vocab, dropout, seed=23):
    from arvae_amd.measure_vae import HierarchicalDecoder
    torch.manual_seed(seed)
    dec = HierarchicalDecoder(10, vocab, 32, 2, hid, dropout).cuda().train()
    with torch.no_grad():                                                   # spread the logits so that the notes vary
        dec.tick_emb_to_note_emb[0].weight.mul_(4.0)
        dec.tick_emb_to_note_emb[0].bias.add_(0.3)
    dec.teacher_forcing_prob = 0.0
    return dec


def test_tick_kernel_distribution(dev, monkeypatch):
    """the same check through the one-launch kernel: 8192 identical latent codes, the first tick's notes against
    softmax(weights[0, 0] / tau)"""
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', '0')
    n, tau = 8192, 1.0
    dec = _decoder(128, 35, 0.5)
    z = torch.from_numpy(syn.normal_noise((1, 32), seed=41)).to(dev).expand(n, -1).contiguous()
    u = library_uniforms(n * 24, 77, 3, dev).view(n, 24)
    weights, samples = dec.generate(z, sampling='multinomial', temperature=tau, uniforms=u)
    assert samples.shape == (n, 1, 24) and dec.training and dec.sampling == 'argmax'
    w0 = weights[0, 0].double().cpu().numpy()
    assert float((weights[:, 0] - weights[0, 0]).abs().max()) <= 1e-5 * float(weights[0, 0].abs().max()) + 1e-6
    chi, kept = chi_square(samples[:, 0, 0].cpu().numpy(), w0, tau)
    print(f'tick kernel distribution: chi-square {chi:.2f} over {kept} bins, critical {CHI2_999[kept - 2]}')
    assert kept >= 8 and chi < CHI2_999[kept - 2]
    assert len(torch.unique(samples[:, 0, 1:])) > 8                        # later ticks follow their own fed-back notes


# ---------------------------------------------------------------- 4. / 5. the one-launch kernel and the per-tick path
TICK_CASES = [(21, 0.0, 128, 35, 1.0),        # 4 rows per workgroup, ragged
              (1501, 0.5, 128, 35, 0.7),      # 8 rows per workgroup
              (2101, 0.0, 64, 35, 1.0),       # 16 rows per workgroup
              (37, 0.5, 64, 16, 1.0),         # one logits tile
              (45, 0.0, 32, 32, 2.0),         # two tiles
              (64, 0.5, 128, 64, 1.0)]        # four tiles, the largest vocabulary
_TICK_RUNS = {}


def tick_run(case, mode, dev, monkeypatch):
    """(tokens (b, 24), weights (b, 24, V) float64, u (b, 24), fraction of band draws, clear rows) of a case in one mode, once"""
    if (case, mode) not in _TICK_RUNS:
        b, dropout, hid, vocab, tau = case
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        dec = _decoder(hid, vocab, dropout)
        dec.sampling, dec.temperature = 'multinomial', tau
        z = torch.from_numpy(syn.normal_noise((b, 32), seed=29)).to(dev)
        u = np.asarray(philox.unit(philox.blocks(b * 24, 1234, 7, 0)[:, 0]), np.float32).reshape(b, 24)
        gen = torch.Generator().manual_seed(4)
        if dropout > 0:
            dec.push_dropout_masks((torch.rand(4, b, hid, generator=gen) >= 0.5).to(torch.uint8).to(dev),
                                   (torch.rand(24, b, hid, generator=gen) >= 0.5).to(torch.uint8).to(dev))
        dec.push_sampling_uniforms(torch.from_numpy(u))
        before = ops.RngState.offset
        with torch.no_grad():
            weights, samples = dec(z, torch.zeros(b, 24, dtype=torch.int64, device=dev), True)
        assert ops.RngState.offset == before                              # every draw was an explicit input
        assert samples.shape == (b, 1, 24) and samples.dtype == torch.int64 and weights.shape == (b, 24, vocab)
        tok = samples[:, 0].cpu().numpy()
        w = weights.double().cpu().numpy()
        assert tok.min() >= 0 and tok.max() < vocab
        eps = 1e-5 * float(np.abs(w).max()) + 1e-6                          # the project's path-against-path bar on the weights
        delta = 2.0 * eps / tau + 1e-5
        band = check_picks(tok, w, u, tau, delta)
        print(f'tick case {case} stepwise {mode}: delta {delta:.3e}, band draws {band:.5f}, distinct notes {len(np.unique(tok))}')
        assert band <= 0.05                                                 # beyond that the test proves nothing
        assert len(np.unique(tok)) > min(8, vocab // 2)
        clear_rows = (pick64(w, u, tau)[1] > delta).all(1)
        _TICK_RUNS[(case, mode)] = (tok, clear_rows)
    return _TICK_RUNS[(case, mode)]


@pytest.mark.parametrize('case', TICK_CASES, ids=[f'b{c[0]}_p{c[1]}_h{c[2]}_v{c[3]}_t{c[4]}' for c in TICK_CASES])
def test_tick_kernel_samples_its_own_weights(dev, monkeypatch, case):
    """every note the one-launch kernel feeds back is the float64 pick from the weights the whole-sequence kernels return for the
    emitted notes, at that tick's uniform (band rule: delta = 2 eps / tau + 1e-5, eps = 1e-5 max|weights| + 1e-6)"""
    tick_run(case, '0', dev, monkeypatch)


@pytest.mark.parametrize('case', TICK_CASES, ids=[f'b{c[0]}_p{c[1]}_h{c[2]}_v{c[3]}_t{c[4]}' for c in TICK_CASES])
def test_per_tick_path_samples_the_same_notes(dev, monkeypatch, case):
    """ARVAE_TICK_STEPWISE=1 (arvae_row_sample per tick) passes the same check, and rows without a band draw in either mode carry
    identical notes in both"""
    tok1, clear1 = tick_run(case, '1', dev, monkeypatch)
    tok0, clear0 = tick_run(case, '0', dev, monkeypatch)
    both = clear0 & clear1
    assert both.mean() > 0.5
    np.testing.assert_array_equal(tok0[both], tok1[both])


# ---------------------------------------------------------------- 6. a training step that samples
def test_training_step_with_multinomial_sampling(dev):
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    b, hid = 37, 128
    torch.manual_seed(11)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, hid, 0.5, 32, 2, hid, 0.5, False, 'folk')
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0, capacity=0.0,
                                rand=0, delta=10.0)
    trainer.cuda()
    model.train()
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
        model.decoder.b_0.fill_(0.1)            # (the beat RNN's constant input: at its initial 0 that layer's input weights get no gradient)
    model.decoder.teacher_forcing_prob = 0.0
    score = torch.from_numpy(syn.measure_batch(b, seed=18)).to(dev)
    eps = torch.from_numpy(syn.normal_noise((b, 32), seed=19))
    gen = torch.Generator().manual_seed(3)
    masks = [(torch.rand(t, b, h, generator=gen) >= 0.5).to(torch.uint8).to(dev) for t, h in ((24, 2 * hid), (4, hid), (24, hid))]
    u1, u2 = (np.asarray(philox.unit(philox.blocks(b * 24, 9, k, 0)[:, 0]), np.float32).reshape(b, 24) for k in (0, 1))

    def push(u):
        model.push_noise(eps)
        model.encoder.push_dropout_mask(masks[0])
        model.decoder.push_dropout_masks(masks[1], masks[2])
        if u is not None:
            model.decoder.push_sampling_uniforms(torch.from_numpy(u))

    def step(u):
        """-> (loss, tokens, gradients, offsets consumed) of forward + step with everything pushed"""
        before = ops.RngState.offset
        push(u)
        with torch.no_grad():
            tokens = model(score, score, train=True)[1].clone()
        trainer.zero_grad()
        push(u)
        loss, _ = trainer.loss_and_acc_for_batch((score, score), 0, 0, True)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        return loss.detach().clone(), tokens, grads, ops.RngState.offset - before

    assert trainer.fused_executor(score) is not None
    argmax_before = step(None)
    model.decoder.sampling = 'multinomial'
    assert trainer.fused_executor(score) is None                           # the whole-model executor keeps declining it
    first, again, other = step(u1), step(u1), step(u2)
    assert torch.isfinite(first[0]) and all(bool(torch.isfinite(g).all()) for g in first[2].values())
    assert [k for k, g in first[2].items() if k.startswith('decoder.') and not float(g.abs().max()) > 0] == []
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert not torch.equal(first[1], other[1]) and not torch.equal(first[1], argmax_before[1])
    assert first[1].shape == (b, 1, 24) and int(first[1].min()) >= 0 and int(first[1].max()) < 35
    # without a pushed buffer a sampled forward draws its uniforms with ONE offset of the library's stream
    consumed = []
    for pushed in (u1, None):
        push(pushed)
        before = ops.RngState.offset
        with torch.no_grad():
            model(score, score, train=True)
        consumed.append(ops.RngState.offset - before)
    assert consumed[1] == consumed[0] + 1
    model.decoder.sampling = 'argmax'
    argmax_after = step(None)
    assert trainer.fused_executor(score) is not None
    assert argmax_after[3] == argmax_before[3] == first[3]                 # sampling with explicit draws consumed no offset either
    assert torch.equal(argmax_before[0], argmax_after[0]) and torch.equal(argmax_before[1], argmax_after[1])
    for k, g in argmax_before[2].items():
        assert torch.equal(g, argmax_after[2][k]), k


# ---------------------------------------------------------------- 7. forward_test
def test_forward_test_matches_forward_on_the_slices(dev):
    from arvae_amd.measure_vae import MeasureVAE
    b, m = 5, 3
    torch.manual_seed(7)
    model = MeasureVAE(_FolkDataset(), 10, 2, 2, 128, 0.5, 32, 2, 128, 0.5, False, 'folk').cuda().eval()
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
    score = torch.from_numpy(syn.measure_batch(b * m, seed=33)).to(dev).view(b, m, 24)
    eps = torch.from_numpy(syn.normal_noise((m * b, 32), seed=34))
    model.push_noise(eps)
    with torch.no_grad():
        weights, samples = model.forward_test(score)
    assert weights.shape == (b, m, 24, 35) and samples.shape == (b, 1, 24 * m) and samples.dtype == torch.int64
    qualifying = 0
    for i in range(m):
        model.push_noise(eps[i * b:(i + 1) * b])
        with torch.no_grad():
            w, s, *_ = model(score[:, i].contiguous(), None, train=False)
        np.testing.assert_allclose(weights[:, i].cpu().numpy(), w.cpu().numpy(), rtol=1e-5, atol=1e-6)
        top2 = torch.topk(w, 2, dim=2).values
        clear = ((top2[..., 0] - top2[..., 1]) > 1e-4).all(1)
        qualifying += int(clear.sum())
        assert torch.equal(samples[:, 0, 24 * i:24 * (i + 1)][clear], s[:, 0][clear])
    assert qualifying >= 0.9 * b * m
    assert len(torch.unique(samples)) > 3


# ---------------------------------------------------------------- 8. the trainer's surface
def test_trainer_decodes_and_samples(dev):
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
    z = torch.randn(6, 16).to(dev)
    before = ops.RngState.offset
    _, notes = trainer.decode_latent_codes(z)
    assert ops.RngState.offset == before
    with torch.no_grad():
        want = model.decoder(z, torch.zeros(6, 24, dtype=torch.int64, device=dev), False)[1]
    assert torch.equal(notes, want)
    u = torch.from_numpy(np.asarray(philox.unit(philox.blocks(6 * 24, 3, 0, 0)[:, 0]), np.float32).reshape(6, 24))
    _, drawn = trainer.decode_latent_codes(z, sampling='multinomial', temperature=1.5, uniforms=u)
    _, drawn_again = trainer.decode_latent_codes(z, sampling='multinomial', temperature=1.5, uniforms=u)
    assert torch.equal(drawn, drawn_again) and not torch.equal(drawn, notes) and not model.training and model.decoder.sampling == 'argmax'
    ops.rng_reseed(21)
    score, first = trainer.sample_measures(16, temperature=0.9)
    _, second = trainer.sample_measures(16, temperature=0.9)
    assert score is None and first.shape == (16, 1, 24) and first.dtype == torch.int64
    assert int(first.min()) >= 0 and int(first.max()) < 35
    assert not torch.equal(first, second)                                   # the stream moves on
    ops.rng_reseed(21)
    assert torch.equal(trainer.sample_measures(16, temperature=0.9)[1], first)         # and restarts with the seed


# ---------------------------------------------------------------- 9. the command line
def _run_cli(args, env_dir):
    env = dict(os.environ, ARVAE_DATA_DIR=str(env_dir), ARVAE_MODEL_DIR=str(env_dir / 'models'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + args, capture_output=True, text=True, timeout=600,
                       env=env, cwd=str(env_dir))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]


def test_cli_sample_flag(dev, tmp_path):
    """--test --sample 4 --temperature 0.8 on a tiny trained checkpoint prints four measures of 24 note names"""
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    common = ['--batch_size', '16', '--rand', '1', '-r', 'all', '--encoder_hidden_size', '64', '--decoder_hidden_size', '64']
    plain = _run_cli(['--num_epochs', '1'] + common, tmp_path)
    assert 'samples' not in plain
    summary = _run_cli(['--test', '--sample', '4', '--temperature', '0.8'] + common, tmp_path)
    assert set(plain) | {'samples'} == set(summary) and summary['num_codes'] == plain['num_codes']
    assert len(summary['samples']) == 4 and all(len(m) == 24 and set(m) <= set(n2i) for m in summary['samples'])

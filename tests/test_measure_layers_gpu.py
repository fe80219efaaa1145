"""MeasureVAE at GRU layer counts other than two on the device: the reference's goldens and the float64 restatement
(tests/layer_stack_ref.py) through the trainer, the layer-count one-launch tick decoder against the tick-by-tick pass, steps with
dropout masks on every layer boundary, the inference entry points, the command line and the executor's fallback."""
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
from oracle import attributes as o_attr
from oracle import philox

import layer_stack_ref as ref
from gru_cases import rows_per_wg
from test_measure_layers import CASE_IDS, LAYER_CASES, _FolkDataset, golden_case, golden_state
from test_sampling import pick64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def close(a, b, rtol=1e-4, atol=0.0):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else b
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def build_trainer(state, enc_layers, dec_layers, hid, dropout=0.0):
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, enc_layers, hid, dropout, 32, dec_layers, hid, dropout, False, 'folk')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0, capacity=0.0,
                                rand=0, delta=10.0)
    trainer.cuda()
    return model, trainer


# ---------------------------------------------------------------- 1. the reference's goldens
@pytest.mark.parametrize('case', LAYER_CASES, ids=CASE_IDS)
def test_layer_step_vs_golden_and_restatement(golden_dir, dev, case):
    """loss_and_acc_for_batch -> backward -> step with the comparisons and tolerances of test_measure_step_vs_golden_and_oracle (the
    float64 restatement in the oracle's place), and the forward's fed-back notes bit-equal to the reference's"""
    enc_layers, dec_layers, hid, batch, mode = case
    g, state, score, eps = golden_case(golden_dir, case)
    teacher, train = mode == 'tf', mode != 'eval'
    model, trainer = build_trainer(state, enc_layers, dec_layers, hid)
    model.train() if train else model.eval()
    model.decoder.teacher_forcing_prob = 1.0 if teacher else 0.0
    st = torch.from_numpy(score).to(dev)
    model.push_noise(torch.from_numpy(eps))
    with torch.no_grad():
        weights, samples, z_dist, _, z, _ = model(st, st, train=train)
    assert weights.shape == (batch, 24, 35) and samples.shape == (batch, 1, 24) and samples.dtype == torch.int64
    np.testing.assert_array_equal(samples.cpu().numpy(), g['samples'])
    close(z, g['z'], rtol=0, atol=1e-4)
    close(z_dist.loc, g['mu'], rtol=0, atol=1e-4)
    close(z_dist.scale, g['sigma'], rtol=1e-4, atol=1e-5)
    w = weights.cpu().numpy()
    close(w[0], g['weights_row0'], rtol=1e-4, atol=1e-5)
    close(w.ravel()[syn.sample_indices('weights', w.size, 128)], g['weights_samp'], rtol=1e-4, atol=1e-5)
    assert trainer.fused_executor(st) is None                   # (the executor is two-layer: these steps take the per-layer path)
    model.push_noise(torch.from_numpy(eps))
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((st, st), 0, 0, train)
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()}
    trainer.step()
    attr = o_attr.attribute_labels(score, *syn.measure_tables())
    want = ref.step(state, score, eps, attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, teacher)
    for src in (g, want):
        close(trainer.last_terms['recons'], float(src['recons']), rtol=1e-4)
        close(trainer.last_terms['dist'], float(src['dist']), rtol=1e-4)
        close(trainer.last_terms['reg'], float(src['reg']), rtol=1e-4)
        close(loss, float(src['loss']), rtol=1e-4)
        close(acc, float(src['acc']), rtol=1e-4)
    for name in state:
        gr = grads[name].astype(np.float64).ravel()
        close(np.sqrt((gr * gr).sum()), float(g[f'gnorm/{name}']), rtol=2e-3)
        wg = want['grads'][name].ravel()
        assert np.linalg.norm(gr - wg) <= 3e-3 * np.linalg.norm(wg) + 1e-9, name
        d = (model.state_dict()[name].cpu().numpy().astype(np.float64) - state[name].astype(np.float64)).ravel()
        close(np.sqrt((d * d).sum()), g[f'dnorm/{name}'], rtol=3e-3)


# ---------------------------------------------------------------- 2. one launch against tick by tick
def spread_model(layers, hid, vocab, dropout, dev, seed=23):
    from arvae_amd.measure_vae import MeasureVAE
    torch.manual_seed(seed)
    ds = _FolkDataset()
    if vocab != 35:                                             # a smaller vocabulary: the first `vocab` symbols
        ds.index2note_dicts = {i: s for i, s in ds.index2note_dicts.items() if i < vocab}
        ds.note2index_dicts = {s: i for s, i in ds.note2index_dicts.items() if i < vocab}
    model = MeasureVAE(ds, 10, 2, layers, hid, dropout, 32, layers, hid, dropout, False, 'folk').cuda().train()
    with torch.no_grad():                                       # spread the logits so that the notes vary
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
    model.decoder.teacher_forcing_prob = 0.0
    return model


def boundary_masks(layers, b, hid, dev, seed=4):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(layers - 1, *shape, generator=gen) >= 0.5).to(torch.uint8).to(dev)
            for shape in ((24, b, 2 * hid), (4, b, hid), (24, b, hid))]


def both_paths(model, layers, b, hid, vocab, dropout, tau, dev, monkeypatch):
    """one forward per path (ARVAE_TICK_STEPWISE 0 / 1) on the same inputs -> {mode: (weights, samples)}, and the uniforms"""
    score = torch.from_numpy(syn.measure_batch(b, seed=28) % vocab).to(dev)
    eps = torch.from_numpy(syn.normal_noise((b, 32), seed=29))
    masks = boundary_masks(layers, b, hid, dev) if dropout > 0 and layers > 1 else None
    u = None
    if tau is not None:
        u = np.asarray(philox.unit(philox.blocks(b * 24, 1234, 7, 0)[:, 0]), np.float32).reshape(b, 24)
    model.decoder.sampling = 'argmax' if tau is None else 'multinomial'
    model.decoder.temperature = 1.0 if tau is None else tau
    out = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        model.push_noise(eps)
        if masks is not None:
            model.encoder.push_dropout_mask(masks[0])
            model.decoder.push_dropout_masks(masks[1], masks[2])
        if u is not None:
            model.decoder.push_sampling_uniforms(torch.from_numpy(u))
        with torch.no_grad():
            weights, samples, *_ = model(score, score, train=True)
        out[mode] = (weights, samples)
    assert not model.encoder._mask_queue and not model.decoder._mask_queue and not model.decoder._uniform_queue
    return out, u


def assert_same_tokens(out, u, tau, b, vocab):
    """argmax: identical token streams.  Multinomial: identical on every row none of whose draws lies within the project's band of a
    CDF bracket boundary in either path (tests/test_sampling_gpu.py: delta = 2 eps / tau + 1e-5, eps = 1e-5 max|weights| + 1e-6 --
    closer than that the two paths' fp32 prefix sums may legitimately fall on either side, and the streams part for good)"""
    t0, t1 = out['0'][1], out['1'][1]
    assert t0.shape == (b, 1, 24) and t0.dtype == torch.int64 and int(t0.min()) >= 0 and int(t0.max()) < vocab
    assert len(torch.unique(t1)) > 3                            # a non-trivial token stream
    if tau is None:
        assert torch.equal(t0, t1)
        close(out['0'][0], out['1'][0], rtol=1e-5, atol=1e-6)
        return
    clear = np.ones(b, bool)
    for mode in ('0', '1'):
        w = out[mode][0].double().cpu().numpy()
        delta = 2.0 * (1e-5 * float(np.abs(w).max()) + 1e-6) / tau + 1e-5
        clear &= (pick64(w, u, tau)[1] > delta).all(1)
    assert clear.mean() > 0.5
    np.testing.assert_array_equal(t0[:, 0].cpu().numpy()[clear], t1[:, 0].cpu().numpy()[clear])


# rows per workgroup of the launcher: 4 up to 1024 rows, 8 up to 2048, 16 beyond; 5 / 1501 / 2101 are ragged against them
# (hidden 128 with three or four layers is not a one-launch shape: test_wide_deep_stacks_decode_tick_by_tick)
TOKEN_CASES = [(layers, hid, vocab, b) for layers in (1, 3) for hid, vocab in ((32, 32), (64, 35), (128, 35)) for b in (5, 20, 1501, 2101)
               if not (layers == 3 and hid == 128)]
TOKEN_CASES += [(4, 64, 35, 20), (4, 64, 35, 1501), (4, 32, 32, 2101)]


@pytest.mark.parametrize('layers,hid,vocab,b', TOKEN_CASES)
def test_tick_layers_tokens_match_stepwise(dev, monkeypatch, layers, hid, vocab, b):
    """the layer-count one-launch tick decoder feeds itself the notes of the launch-per-tick pass: with and without keep-masks on every
    layer boundary, top-1 feedback and multinomial feedback at explicit uniforms (T = 1 and 0.7)"""
    assert ops.tick_free_run_layers_supported(hid, vocab, layers)
    for dropout, tau in [(dropout, tau) for dropout in (0.0, 0.5) for tau in (None, 1.0, 0.7)]:
        model = spread_model(layers, hid, vocab, dropout, dev)
        out, u = both_paths(model, layers, b, hid, vocab, dropout, tau, dev, monkeypatch)
        assert_same_tokens(out, u, tau, b, vocab)
        if b > 1024:                                            # the one-launch pass again: a run-to-run difference is a fault
            again, _ = both_paths(model, layers, b, hid, vocab, dropout, tau, dev, monkeypatch)
            assert torch.equal(again['0'][1], out['0'][1])


@pytest.mark.parametrize('b', [5, 20, 1029, 2053])
def test_two_layer_tokens_match_stepwise_at_hidden_32(dev, monkeypatch, b):
    """the two-layer one-launch decoder (tick_free_run_h2_kernel behind the shared weight prep) at its smallest shape, which the 35-note
    vocabulary does not reach: hidden 32 has one k-step and nine weight groups per tick, so the register ring is 3 deep instead of 6.
    1029 and 2053 rows: 8 and 16 rows per workgroup (gru_rows_per_wg for one sequence), five rows in the last workgroup"""
    assert ops.tick_free_run_supported(32, 32)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = {5: 4, 20: 4, 1029: 8, 2053: 16}[b]
    assert rows_per_wg(b, 1, cus) == want, \
        f'{b} rows on {cus} CUs run {rows_per_wg(b, 1, cus)} rows per workgroup: this case is written for {want} (256 CUs)'
    for dropout, tau in [(dropout, tau) for dropout in (0.0, 0.5) for tau in (None, 1.0, 0.7)]:
        model = spread_model(2, 32, 32, dropout, dev)
        out, u = both_paths(model, 2, b, 32, 32, dropout, tau, dev, monkeypatch)
        assert_same_tokens(out, u, tau, b, 32)


@pytest.mark.parametrize('layers,b,dropout,hid', [(1, 64, 0.5, 128), (3, 64, 0.5, 64), (3, 45, 0.0, 64), (1, 45, 0.0, 64)])
def test_tick_layers_tokens_match_stepwise_big(dev, monkeypatch, layers, b, dropout, hid):
    """the `big` scaling case of test_tick_free_run_tokens_match_stepwise: initial tick states of ~1e4 and recurrent tick weights of ~350,
    which only operand scales taken from the data can hold in fp16"""
    model = spread_model(layers, hid, 35, dropout, dev)
    with torch.no_grad():
        model.decoder.beat_emb_to_tick_rnn_hidden[0].weight.mul_(20000.0)
        for k in range(layers):
            getattr(model.decoder.rnn_tick, f'weight_hh_l{k}').mul_(4000.0)
            if k > 0:
                getattr(model.decoder.rnn_tick, f'weight_ih_l{k}').mul_(4000.0)
        assert float(model.decoder.rnn_tick.weight_hh_l0.abs().max()) > 255.0
    out, u = both_paths(model, layers, b, hid, 35, dropout, None, dev, monkeypatch)
    assert_same_tokens(out, u, None, b, 35)


def test_wide_deep_stacks_decode_tick_by_tick(dev, monkeypatch):
    """hidden 128 with three (or four) layers is not offered as one launch: the decoder takes the tick-by-tick pass and the library
    refuses the shape"""
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', '0')
    assert not ops.tick_free_run_layers_supported(128, 35, 3) and not ops.tick_free_run_layers_supported(128, 35, 4)
    model = spread_model(3, 128, 35, 0.0, dev)
    seen = []
    monkeypatch.setattr(ops, 'tick_free_run_layers', lambda *a, **k: seen.append(1))
    score = torch.from_numpy(syn.measure_batch(5, seed=28)).to(dev)
    with torch.no_grad():
        weights, samples, *_ = model(score, score, train=True)
    assert not seen and samples.shape == (5, 1, 24) and int(samples.min()) >= 0 and int(samples.max()) < 35
    assert torch.equal(samples[:, 0], weights.argmax(2))          # the notes are the top-1 of the weights the forward returns


def test_tick_layers_op_checks_its_inputs(dev):
    cells = [tuple(torch.zeros(s, device=dev) for s in ((192, 64), (192, 64), (192,), (192,))) for _ in range(3)]
    h0 = [torch.zeros(4 * 5, 64, device=dev) for _ in range(3)]
    args = (torch.zeros(35, 64, device=dev), torch.zeros(35, device=dev))
    gib, ptab = torch.zeros(20, 192, device=dev), torch.zeros(36, 192, device=dev)
    tokens = ops.tick_free_run_layers(cells, *args, h0, gib, ptab, None, 1.0, 5, 4, 6)
    assert tokens.shape == (5, 24) and int(tokens.abs().max()) == 0             # all-zero logits: the lowest index
    with pytest.raises(ValueError):
        ops.tick_free_run_layers(cells, *args, h0[:2], gib, ptab, None, 1.0, 5, 4, 6)
    with pytest.raises(ValueError):                              # one mask for two boundaries
        ops.tick_free_run_layers(cells, *args, h0, gib, ptab, torch.ones(1, 24, 5, 64, dtype=torch.uint8, device=dev), 2.0, 5, 4, 6)
    with pytest.raises(RuntimeError):                            # two layers: arvae_tick_free_run
        ops.tick_free_run_layers(cells[:2], *args, h0[:2], gib, ptab, None, 1.0, 5, 4, 6)


# ---------------------------------------------------------------- 3. a training step with masks on every boundary
@pytest.mark.parametrize('teacher', [True, False], ids=['tf', 'free'])
def test_masked_train_step_vs_restatement(dev, teacher):
    """L = 3, H = 64, B = 20, dropout 0.5 with explicit keep-masks on both boundaries of all three RNNs against the float64
    restatement: losses at rtol 1e-4, z at atol 1e-4, gradients at the MeasureVAE bar (3e-3 of the reference gradient's L2 norm).
    Noise seed 43 and mask seed 8 leave a top-1 margin of 2.5e-3 in the free-running pass (asserted: > 1e-4)."""
    layers, hid, b = 3, 64, 20
    state = golden_state(layers, layers, hid)
    score = syn.measure_batch(b, seed=5)
    eps = syn.normal_noise((b, 32), seed=43)
    enc_m, beat_m, tick_m = syn.dropout_masks([(2, 24, b, 2 * hid), (2, 4, b, hid), (2, 24, b, hid)], 8)
    attr = o_attr.attribute_labels(score, *syn.measure_tables())
    want = ref.step(state, score, eps, attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, teacher, dict(enc=enc_m, beat=beat_m, tick=tick_m))
    top2 = np.sort(want['weights'], -1)[..., -2:]
    assert (top2[..., 1] - top2[..., 0]).min() > 1e-4
    model, trainer = build_trainer(state, layers, layers, hid, dropout=0.5)
    model.train()
    model.decoder.teacher_forcing_prob = 1.0 if teacher else 0.0
    st = torch.from_numpy(score).to(dev)
    outs = []
    for _ in range(2):                                           # the forward alone (z, notes), then the trainer's step
        model.push_noise(torch.from_numpy(eps))
        model.encoder.push_dropout_mask(torch.from_numpy(enc_m).to(dev))
        model.decoder.push_dropout_masks(torch.from_numpy(beat_m).to(dev), torch.from_numpy(tick_m).to(dev))
        if not outs:
            with torch.no_grad():
                outs = model(st, st, train=True)
    weights, samples, _, _, z, _ = outs
    np.testing.assert_array_equal(samples.cpu().numpy(), want['samples'])
    close(z, want['z'], rtol=0, atol=1e-4)
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((st, st), 0, 0, True)
    loss.backward()
    for k in ('recons', 'dist', 'reg'):
        close(trainer.last_terms[k], want[k], rtol=1e-4)
    close(loss, want['loss'], rtol=1e-4)
    close(acc, want['acc'], rtol=1e-4)
    for name, p in model.named_parameters():
        gr, wg = p.grad.detach().cpu().numpy().astype(np.float64).ravel(), want['grads'][name].ravel()
        assert np.linalg.norm(gr - wg) <= 3e-3 * np.linalg.norm(wg) + 1e-9, name


def test_device_drawn_masks_take_one_offset_per_boundary(dev):
    """without pushed masks a training forward draws, per RNN group, one keep-mask per layer boundary: Philox offsets in the order
    encoder boundaries, eps, decoder boundaries (L = 3: 2 + 1 + 2; L = 1: eps alone; two layers keep their 1 + 1 + 1)"""
    for layers, draws in ((1, 1), (2, 3), (3, 5)):
        model = spread_model(layers, 64, 35, 0.5, dev)
        model.decoder.teacher_forcing_prob = 1.0
        score = torch.from_numpy(syn.measure_batch(6, seed=3)).to(dev)
        before = ops.RngState.offset
        with torch.no_grad():
            model(score, score, train=True, need_prior_sample=False)
        assert ops.RngState.offset - before == draws, layers


# ---------------------------------------------------------------- 4. inference entry points
@pytest.mark.parametrize('layers', [1, 3])
def test_generate_forward_test_and_sampling(dev, layers):
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    b, m = 5, 3
    model = spread_model(layers, 64, 35, 0.5, dev, seed=7).eval()
    z = torch.from_numpy(syn.normal_noise((6, 32), seed=41)).to(dev)
    dummy = torch.zeros(6, 24, dtype=torch.int64, device=dev)
    with torch.no_grad():
        want_w, want = model.decoder(z, dummy, False)
    w, notes = model.decoder.generate(z, sampling='argmax')
    assert torch.equal(notes, want) and torch.equal(w, want_w) and not model.decoder.training
    u = torch.from_numpy(np.asarray(philox.unit(philox.blocks(6 * 24, 3, 0, 0)[:, 0]), np.float32).reshape(6, 24))
    _, drawn = model.decoder.generate(z, sampling='multinomial', temperature=1.5, uniforms=u)
    _, again = model.decoder.generate(z, sampling='multinomial', temperature=1.5, uniforms=u)
    assert torch.equal(drawn, again) and not torch.equal(drawn, notes) and int(drawn.max()) < 35 and int(drawn.min()) >= 0
    # forward_test: every measure's slice is the plain evaluation forward of that measure
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
            wi, si, *_ = model(score[:, i].contiguous(), None, train=False)
        close(weights[:, i], wi, rtol=1e-5, atol=1e-6)
        top2 = torch.topk(wi, 2, dim=2).values
        clear = ((top2[..., 0] - top2[..., 1]) > 1e-4).all(1)
        qualifying += int(clear.sum())
        assert torch.equal(samples[:, 0, 24 * i:24 * (i + 1)][clear], si[:, 0][clear])
    assert qualifying >= 0.9 * b * m
    # the trainer's sampler
    ds = _FolkDataset()
    trainer = MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))
    trainer.cuda()
    model.eval()
    ops.rng_reseed(21)
    score_none, first = trainer.sample_measures(16, temperature=0.9)
    assert score_none is None and first.shape == (16, 1, 24) and first.dtype == torch.int64
    assert int(first.min()) >= 0 and int(first.max()) < 35 and len(torch.unique(first)) > 3
    ops.rng_reseed(21)
    assert torch.equal(trainer.sample_measures(16, temperature=0.9)[1], first)


# ---------------------------------------------------------------- 5. the executor's fallback
def test_trainer_reports_the_layer_count_and_takes_the_per_layer_path(dev):
    from arvae_amd.fused_measure import FusedMeasureVAE
    state = golden_state(3, 1, 64)
    score = torch.from_numpy(syn.measure_batch(20, seed=5)).to(dev)
    eps = torch.from_numpy(syn.normal_noise((20, 32), seed=41))
    res = {}
    for fused in (True, False):
        model, trainer = build_trainer(state, 3, 1, 64)
        trainer.use_fused_step = fused
        model.train()
        model.decoder.teacher_forcing_prob = 0.0
        if fused:
            assert FusedMeasureVAE.supports(model, trainer.optimizer, (0, 1, 2, 3)) == 'layer count not built in the executor'
        assert trainer.fused_executor(score) is None
        model.push_noise(eps)
        trainer.zero_grad()
        loss, acc = trainer.loss_and_acc_for_batch((score, score), 0, 0, True)
        loss.backward()
        trainer.step()
        res[fused] = (float(loss), float(acc), {k: v.detach().clone() for k, v in model.state_dict().items()})
    assert res[True][0] == res[False][0] and res[True][1] == res[False][1]
    for k, v in res[False][2].items():
        assert torch.equal(res[True][2][k], v), k


# ---------------------------------------------------------------- 6. the command line
def _run_cli(args, env_dir):
    env = dict(os.environ, ARVAE_DATA_DIR=str(env_dir), ARVAE_MODEL_DIR=str(env_dir / 'models'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + args, capture_output=True, text=True, timeout=600,
                       env=env, cwd=str(env_dir))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]


def test_cli_with_other_layer_counts(dev, tmp_path):
    """--num_encoder_layers 3 --num_decoder_layers 1: two tiny epochs, the checkpoint with its extra keys, --test reloading it, --sample"""
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    common = ['--batch_size', '16', '--rand', '1', '-r', 'all', '--encoder_hidden_size', '64', '--decoder_hidden_size', '64',
              '--num_encoder_layers', '3', '--num_decoder_layers', '1']
    trained = _run_cli(['--num_epochs', '2'] + common, tmp_path)
    assert trained['attributes'] == ['rhy_complexity', 'pitch_range', 'note_density', 'contour']
    assert trained['num_codes'] == 16 and np.isfinite(trained['test_loss']) and 'samples' not in trained
    name = trained['model']
    saved = torch.load(tmp_path / 'models' / name / (name + '.pt'), map_location='cpu')
    assert [[k, list(v.shape)] for k, v in saved.items()] == [[k, list(s)] for k, s in ref.shapes(3, 1, 64).items()]
    again = _run_cli(['--test', '--sample', '4'] + common, tmp_path)
    assert again['model'] == name and again['num_codes'] == 16
    assert again['test_loss'] == pytest.approx(trained['test_loss'], rel=5e-2)          # eps is redrawn
    assert len(again['samples']) == 4 and all(len(m) == 24 and set(m) <= set(n2i) for m in again['samples'])

"""MeasureVAE at hidden sizes 256 and 512 -- the class's own default among them -- on the whole-sequence path (csrc/gru_wide.hip)
against the launch-per-time-step path (ARVAE_GRU_STEPWISE=1), and the scratch contract of the wide entry points.  Needs a real
MI355X.

Tolerances are those of test_measure_sequence_path_matches_stepwise (test_hip_parity.py): loss rtol 1e-5, accuracy 1e-6, every
gradient within 2e-4 of its norm."""
import pytest
import torch

import guarded_alloc as ga
from arvae_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GAP = 1e-4                                 # free running: the two largest logits of the stepwise pass at every (row, tick)
SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)   # model seeds tried in this order; the first whose stepwise pass keeps GAP is used


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


class _FolkDataset:
    """the attributes MeasureVAE / MeasureVAETrainer read from the reference's FolkNBarDataset"""
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


def close(a, b, rtol):
    assert abs(a - b) <= rtol * abs(b), (a, b, rtol)


def _masks(b, enc_hid, dec_hid, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(24, b, 2 * enc_hid, generator=gen) >= 0.5).to(torch.uint8),
            (torch.rand(4, b, dec_hid, generator=gen) >= 0.5).to(torch.uint8),
            (torch.rand(24, b, dec_hid, generator=gen) >= 0.5).to(torch.uint8)]


def _build(seed, make, dev):
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    torch.manual_seed(seed)
    ds = _FolkDataset()
    model = make(ds)
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0, capacity=0.0, rand=0,
                                delta=10.0)
    trainer.cuda()
    model.train()
    return model, trainer


def _push(model, eps, masks, dev):
    model.push_noise(eps)
    model.encoder.push_dropout_mask(masks[0].to(dev))
    model.decoder.push_dropout_masks(masks[1].to(dev), masks[2].to(dev))


def _step(monkeypatch, mode, seed, make, teacher, score, eps, masks, dev, spread=False):
    """one loss + backward in `mode` ('0' sequences, '1' stepwise) -> (loss, accuracy, gradients, logits (B, 24, V), fed-back tokens)"""
    monkeypatch.setenv('ARVAE_GRU_STEPWISE', mode)
    model, trainer = _build(seed, make, dev)
    if spread:                                                  # spread the logits so that the argmax varies over the ticks
        with torch.no_grad():
            model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
            model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
    model.decoder.teacher_forcing_prob = 1.0 if teacher else 0.0
    _push(model, eps, masks, dev)
    with torch.no_grad():
        weights, samples = model(score, None, True, need_prior_sample=False)[:2]
    _push(model, eps, masks, dev)
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((score, score), 0, 0, True)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and bool(torch.isfinite(loss.detach()))
    return float(loss.detach()), float(acc), grads, weights.detach(), samples.detach().reshape(score.shape[0], 24)


def _agree(what, seq, step):
    close(seq[0], step[0], 1e-5)
    close(seq[1], step[1], 1e-6)
    for k, gstep in step[2].items():
        gseq = seq[2][k]
        assert float((gseq - gstep).norm()) <= 2e-4 * float(gstep.norm()) + 1e-9, (what, k, float((gseq - gstep).norm()), float(gstep.norm()))


def _wide(ds):
    from arvae_amd.measure_vae import MeasureVAE
    return MeasureVAE(ds, 10, 2, 2, 256, 0.5, 32, 2, 512, 0.5, False, 'folk')


def _inputs(b, zdim, enc_hid, dec_hid, dev):
    score = torch.from_numpy(syn.measure_batch(b, seed=18)).to(dev)
    eps = torch.from_numpy(syn.normal_noise((b, zdim), seed=19))
    return score, eps, _masks(b, enc_hid, dec_hid, 3)


def test_teacher_forced_matches_stepwise(dev, monkeypatch):
    """encoder 256, decoder 512, latent 32, 21 measures, explicit noise and keep-masks (24, 21, 512), (4, 21, 512), (24, 21, 512)"""
    score, eps, masks = _inputs(21, 32, 256, 512, dev)
    assert [tuple(m.shape) for m in masks] == [(24, 21, 512), (4, 21, 512), (24, 21, 512)]
    res = {mode: _step(monkeypatch, mode, 11, _wide, True, score, eps, masks, dev) for mode in ('0', '1')}
    assert torch.equal(res['0'][4], score) and torch.equal(res['1'][4], score)
    _agree('teacher forced', res['0'], res['1'])


def test_free_running_matches_stepwise(dev, monkeypatch):
    """the same model feeding itself.  The fed-back note is an argmax, so the comparison needs a problem on which it cannot flip: the
    model seed is the first of SEEDS for which the stepwise pass's two largest logits are at least GAP apart at every (row, tick) of
    all 21 rows (asserted), both modes are then held to have fed back the same tokens, and only then are losses and gradients
    compared.  No row is dropped and no tolerance moves."""
    score, eps, masks = _inputs(21, 32, 256, 512, dev)
    step = seed = None
    for s in SEEDS:
        cand = _step(monkeypatch, '1', s, _wide, False, score, eps, masks, dev, spread=True)
        top2 = torch.topk(cand[3], 2, dim=-1).values
        gap = float((top2[..., 0] - top2[..., 1]).min())
        print(f'seed {s}: smallest gap between the two largest logits over 21 x 24 ticks {gap:.3e}')
        if gap >= GAP:
            step, seed = cand, s
            break
    assert step is not None, f'no seed of {SEEDS} keeps the two largest logits {GAP} apart on all 21 rows'
    top2 = torch.topk(step[3], 2, dim=-1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= GAP
    assert int(step[4].unique().numel()) > 1                   # the argmax varies
    seq = _step(monkeypatch, '0', seed, _wide, False, score, eps, masks, dev, spread=True)
    assert torch.equal(seq[4], step[4]), 'the two modes fed back different tokens'
    print(f'free running: seed {seed}, 21 of 21 rows')
    _agree('free running', seq, step)


def test_class_default_runs_on_the_wide_entry_points(dev, monkeypatch):
    """MeasureVAE(dataset) as the class (and the reference) builds it -- 512 / 512, latent 256 -- on 5 measures: one teacher-forced
    training step is finite, agrees with the stepwise path, and its six GRU layers (two encoder layers of two directions each, two
    beat and two tick layers) each went through arvae_gru_seq_wide_fwd exactly once."""
    from arvae_amd import _lib
    from arvae_amd.measure_vae import MeasureVAE
    make = lambda ds: MeasureVAE(ds)                            # noqa: E731
    probe = make(_FolkDataset())
    assert (probe.encoder_hidden_size, probe.decoder_hidden_size, probe.latent_space_dim) == (512, 512, 256)
    score, eps, masks = _inputs(5, 256, 512, 512, dev)
    lib = _lib.load()
    real, calls = lib.arvae_gru_seq_wide_fwd, []

    def counted(descs, nseq, steps, rows, hid, ws, stream):
        calls.append((nseq, steps, rows, hid))
        return real(descs, nseq, steps, rows, hid, ws, stream)

    monkeypatch.setattr(lib, 'arvae_gru_seq_wide_fwd', counted)
    seq = _step(monkeypatch, '0', 11, make, True, score, eps, masks, dev)
    n_forward_pass = len(calls) // 2                            # _step runs the forward twice: once for the logits, once for the loss
    assert len(calls) == 12 and calls[:n_forward_pass] == calls[n_forward_pass:], calls
    assert sorted(calls[:6]) == sorted([(2, 24, 5, 512)] * 2 + [(1, 4, 5, 512)] * 2 + [(1, 6, 20, 512)] * 2), calls
    step = _step(monkeypatch, '1', 11, make, True, score, eps, masks, dev)
    assert len(calls) == 12                                     # the stepwise path never comes here
    _agree('class default', seq, step)


def test_a_captured_graph_holds_the_wide_calls(dev):
    """HIP-graph replay of a 256 / 256 model's forward + backward (arvae_amd.graphed: the per-layer path, every GRU layer a wide call
    of one launch per time step) against the eager step, on other data than it was captured on: the entry points neither allocate
    nor synchronise nor read back, and the same kernels in the same order give a bit-identical loss and gradient arena
    (test_graphed_measure_step_matches_eager's method: dropout off, fixed noise buffer, the decoder's coin pinned both ways)."""
    from arvae_amd.graphed import GraphedStep
    from arvae_amd.measure_vae import MeasureVAE
    model, trainer = _build(0, lambda ds: MeasureVAE(ds, 10, 2, 2, 256, 0.0, 16, 2, 256, 0.0, False, 'folk'), dev)
    b = 32
    model.encoder.static_eps = torch.from_numpy(syn.normal_noise((b, 16), seed=3)).to(dev)
    score = torch.from_numpy(syn.measure_batch(b, seed=8)).to(dev)
    other = torch.from_numpy(syn.measure_batch(b, seed=9)).to(dev)
    try:
        graphed = GraphedStep(trainer, (other, other))
        for forced in (True, False):
            model.decoder.teacher_forcing_prob = 2.0 if forced else -1.0
            trainer.zero_grad()
            loss, _ = trainer.loss_and_acc_for_batch((score, score), 0, 1, True)
            loss.backward()
            want_loss, want_grad = float(loss.detach()), trainer.optimizer.grad_arena.clone()
            graphed.prob = 2.0 if forced else -1.0
            got_loss, _ = graphed((score, score))
            torch.cuda.synchronize()
            assert float(got_loss) == want_loss, forced
            assert torch.equal(trainer.optimizer.grad_arena, want_grad), forced
    finally:
        type(model.encoder).static_eps = None
        model.encoder.static_eps = None


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def test_scratch_contract(dev, monkeypatch):
    """one forward and backward of a 256-wide ops.gru_sequence (two sequences, 37 rows, 6 steps, initial states: the backward's tail
    launch runs) with every torch.empty of ops guarded and poisoned, 0xFF and then 0x7E: both guard bands of every allocation
    intact -- the workspace's among them --, nothing passed the proxy by, results bit-identical to the plain run"""
    from arvae_amd import ops
    import numpy as np
    hid, steps, rows = 256, 6, 37
    rs = np.random.RandomState(256)
    k = 1.0 / np.sqrt(hid)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)      # noqa: E731
    gi, h0 = f32(rs.standard_normal((2, steps, rows, 3 * hid))), f32(rs.uniform(-1, 1, (2, rows, hid)))
    w, bh = f32(rs.uniform(-k, k, (2, 3 * hid, hid))), f32(rs.uniform(-k, k, (2, 3 * hid)))
    d_out, d_fin = f32(rs.standard_normal((steps, rows, 2 * hid))), f32(rs.standard_normal((rows, 2 * hid)))

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (gi[0], gi[1], h0[0], h0[1], w[0], w[1], bh[0], bh[1])]
        g0, g1, a0, a1, w0, w1, b0, b1 = leaves
        out, fin = ops.gru_sequence(steps, [(g0, w0, b0, a0, False), (g1, w1, b1, a1, True)])
        ((out * d_out).sum() + (fin * d_fin).sum()).backward()
        torch.cuda.synchronize()
        return [out.detach(), fin.detach()] + [t.grad for t in leaves]

    plain = run()
    for fill in (ga.FILL_NAN, ga.FILL_BIG):
        with monkeypatch.context() as m:
            proxy = ga.GuardedTorch(fill).install(m, ops)
            got = run()
        proxy.check_bands()
        assert proxy.passed_through == [] and proxy.records
        assert any('_gru_seq_call' in rec.site for rec in proxy.records), proxy.by_site()
        for i, (a, b) in enumerate(zip(got, plain)):
            assert bool(torch.isfinite(a).all()), (fill, i)
            assert int((_bits(a) != _bits(b)).sum()) == 0, (fill, i)

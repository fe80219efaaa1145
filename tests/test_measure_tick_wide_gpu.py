"""MeasureVAE's free-running decode at hidden sizes 256 and 512 through the one call of csrc/tick_wide.hip against the tick-by-tick
pass (ARVAE_TICK_STEPWISE=1), at model level: `generate` in its four pick forms, the class default's call count, and a captured
graph.  Needs a real MI355X.  After test_measure_wide_gpu.py: its model (encoder 256, decoder 512, latent 32), 21 measures, its
GAP and seed search.

The two passes form a tick's logits with different GEMMs (one kernel with the input projection folded into a table against
dense + gates launches), so their logits differ in the last bits and a pick is only comparable where it cannot flip:
  argmax, planned argmax   the model seed is the first of SEEDS for which the stepwise pass's two largest ALLOWED logits are at least
                           GAP apart at every (row, tick) of all 21 rows (asserted); no row is dropped;
  multinomial, filtered    the stepwise pass runs first, and the uniforms are made on the host from ITS logits so that every draw is
                           at least MARGIN from the nearest boundary of that (row, tick)'s CDF (asserted on the final stepwise pass).
                           A draw that is closer is moved to the middle of the widest interval of its CDF and the stepwise pass
                           runs again: ticks before the earliest moved draw of a row repeat exactly, so this ends.  With a top-k cut
                           the k-th and (k+1)-th allowed logits are GAP apart as well (asserted; the seed search).
Then both passes must emit identical tokens, and the weights -- the teacher-forced kernels on those tokens in either pass -- agree
to rtol 1e-5 of the largest weight."""
import numpy as np
import pytest
import torch

from arvae_amd import synthetic as syn
from test_measure_wide_gpu import GAP, SEEDS, _FolkDataset, _build, _wide

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
B = 21


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _decoder(seed, dev):
    model, _ = _build(seed, _wide, dev)
    with torch.no_grad():                                       # spread the logits so that the picks vary over the ticks
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
    return model.decoder


def _codes(dev, b=B, zdim=32):
    return torch.from_numpy(syn.normal_noise((b, zdim), seed=19)).to(dev)


def _generate(monkeypatch, stepwise, dec, z, **kw):
    monkeypatch.setenv('ARVAE_TICK_STEPWISE', '1' if stepwise else '0')
    monkeypatch.delenv('ARVAE_GRU_STEPWISE', raising=False)
    weights, samples = dec.generate(z, **kw)
    torch.cuda.synchronize()
    return weights.detach(), samples.detach().reshape(z.shape[0], 24)


def _same(what, new, step):
    assert torch.equal(new[1], step[1]), f'{what}: the two passes emitted different tokens'
    assert float((new[0] - step[0]).abs().max()) <= 1e-5 * float(step[0].abs().max()), what


def _plan(vocab, seed):
    """(B, 24, V) flags: every fourth tick forces one note, the others allow about half of the vocabulary (two notes at least)"""
    rs = np.random.RandomState(seed)
    plan = (rs.uniform(size=(B, 24, vocab)) < 0.5).astype(np.uint8)
    for b in range(B):
        for t in range(24):
            if t % 4 == 1:
                plan[b, t] = 0
                plan[b, t, rs.randint(vocab)] = 1
            else:
                plan[b, t, rs.choice(vocab, 2, replace=False)] = 1
    return plan


def _allowed_gap(weights, on):
    """the smallest distance between the two largest allowed logits over the (row, tick)s that allow two notes at least"""
    w = weights.double().cpu()
    w = torch.where(on, w, torch.full_like(w, -float('inf')))
    top2 = torch.topk(w, 2, dim=-1).values
    several = on.sum(-1) >= 2
    return float((top2[..., 0] - top2[..., 1])[several].min())


@pytest.mark.parametrize('planned', [False, True], ids=['argmax', 'planned-argmax'])
def test_generate_argmax_matches_stepwise(dev, monkeypatch, planned):
    z = _codes(dev)
    vocab = len(_FolkDataset().note2index_dicts)
    plan = _plan(vocab, 5) if planned else None
    on = torch.from_numpy(plan != 0) if planned else torch.ones(B, 24, vocab, dtype=torch.bool)
    step = dec = None
    for s in SEEDS:
        cand_dec = _decoder(s, dev)
        cand = _generate(monkeypatch, True, cand_dec, z, sampling='argmax', plan=plan)
        gap = _allowed_gap(cand[0], on)
        print(f'seed {s}: smallest gap between the two largest allowed logits over {B} x 24 ticks {gap:.3e}')
        if gap >= GAP:
            step, dec = cand, cand_dec
            break
    assert step is not None, f'no seed of {SEEDS} keeps the two largest allowed logits {GAP} apart on all {B} rows'
    assert _allowed_gap(step[0], on) >= GAP
    assert int(step[1].unique().numel()) > 1                    # the argmax varies
    if planned:
        assert bool(torch.gather(torch.from_numpy(plan).to(dev), 2, step[1][:, :, None]).ne(0).all())
    new = _generate(monkeypatch, False, dec, z, sampling='argmax', plan=plan)
    _same('planned argmax' if planned else 'argmax', new, step)


def _cdf(weights, inv_t, top_k, allow):
    """on the host in float64, per (row, tick): the CDF over the notes in index order, C_k / C_last (a note that does not survive keeps
    the value before it), and the distance between the k-th and (k+1)-th allowed logits (inf without a top-k cut)"""
    l = weights.double().cpu().numpy()
    on = np.ones(l.shape[-1], bool) if allow is None else np.asarray(allow) != 0
    lm = np.where(on, l, -np.inf)
    kept = np.broadcast_to(on, l.shape).copy()
    cut_gap = np.full(l.shape[:2], np.inf)
    if top_k is not None:
        order = np.argsort(-lm, axis=-1, kind='stable')         # descending logit, ties to the lower index
        rank = np.argsort(order, axis=-1, kind='stable')
        kept &= rank < top_k
        ordered = np.take_along_axis(lm, order, -1)
        cut_gap = ordered[..., top_k - 1] - ordered[..., top_k]
    e = np.where(kept, np.exp((l - np.where(kept, l, -np.inf).max(-1, keepdims=True)) * inv_t), 0.0)
    c = np.cumsum(e, -1)
    return c / c[..., -1:], cut_gap


def _settled_uniforms(monkeypatch, dec, z, temperature, top_k, allow, seed):
    """-> (uniforms (B, 24) on the host, the stepwise pass run with them, the smallest distance of a draw to a CDF boundary, the smallest
    top-k distance), or None when 24 rounds do not settle them"""
    u = 1.0 - np.random.RandomState(seed).uniform(size=(B, 24))
    kw = dict(sampling='multinomial', temperature=temperature, top_k=top_k, allowed=allow)
    for _ in range(25):
        step = _generate(monkeypatch, True, dec, z, uniforms=torch.from_numpy(u.astype(np.float32)).to(z.device), **kw)
        u = u.astype(np.float32).astype(np.float64)             # the draws as the kernels read them
        cdf, cut_gap = _cdf(step[0], 1.0 / temperature, top_k, allow)
        edges = np.concatenate((np.zeros_like(cdf[..., :1]), cdf), -1)
        dist = np.abs(u[..., None] - edges).min(-1)
        bad = dist < MARGIN
        if not bad.any():
            return u.astype(np.float32), step, float(dist.min()), float(cut_gap.min())
        width = np.diff(edges, axis=-1)
        k = width.argmax(-1)
        mid = np.take_along_axis(edges, k[..., None], -1)[..., 0] + 0.5 * np.take_along_axis(width, k[..., None], -1)[..., 0]
        u = np.where(bad, mid, u)
    return None


@pytest.mark.parametrize('filtered', [False, True], ids=['multinomial', 'filtered'])
def test_generate_draws_match_stepwise(dev, monkeypatch, filtered):
    z = _codes(dev)
    vocab = len(_FolkDataset().note2index_dicts)
    top_k, allow = None, None
    if filtered:
        top_k = 4
        allow = (np.random.RandomState(6).uniform(size=vocab) < 0.7).astype(np.uint8)
        allow[:8] = 1
    found = None
    for s in SEEDS:
        dec = _decoder(s, dev)
        got = _settled_uniforms(monkeypatch, dec, z, 0.8, top_k, allow, seed=s)
        if got is None:
            print(f'seed {s}: the draws did not settle')
            continue
        print(f'seed {s}: smallest distance of a draw to a CDF boundary {got[2]:.3e}, of the top-k cut\'s two logits {got[3]:.3e}')
        if got[3] >= GAP:
            found = (dec,) + got
            break
    assert found is not None, f'no seed of {SEEDS} gives draws {MARGIN} from every CDF boundary' + (f' and a top-k cut {GAP} wide' if filtered else '')
    dec, u, step, dist, cut_gap = found
    assert dist >= MARGIN and cut_gap >= GAP                    # made from, and held against, the stepwise pass's own logits
    assert u.min() > 0 and u.max() <= 1 and int(step[1].unique().numel()) > 2
    if filtered:
        assert bool((torch.from_numpy(allow).to(dev)[step[1]] != 0).all())
    new = _generate(monkeypatch, False, dec, z, sampling='multinomial', temperature=0.8, top_k=top_k, allowed=allow,
                    uniforms=torch.from_numpy(u).to(dev))
    _same('filtered' if filtered else 'multinomial', new, step)


def test_class_default_generates_in_one_call(dev, monkeypatch):
    """MeasureVAE(dataset) as the class (and the reference) builds it -- 512 / 512, latent 256 --, 5 measures: one `generate` goes through
    arvae_tick_free_run_wide exactly once and through no arvae_row_* symbol"""
    from arvae_amd import _lib
    from arvae_amd.measure_vae import MeasureVAE
    model, _ = _build(11, lambda ds: MeasureVAE(ds), dev)
    assert (model.decoder_hidden_size, model.latent_space_dim) == (512, 256)
    lib = _lib.load()
    calls = {}

    def counted(name):
        real = getattr(lib, name)

        def call(*a):
            calls[name] = calls.get(name, 0) + 1
            return real(*a)
        return call

    rows = [n for n in _lib.SIGNATURES if n.startswith('arvae_row_')]
    assert {'arvae_row_argmax', 'arvae_row_sample', 'arvae_row_sample_filtered', 'arvae_row_sample_planned'} <= set(rows)
    for name in rows + ['arvae_tick_free_run_wide']:
        monkeypatch.setattr(lib, name, counted(name))
    z = _codes(dev, 5, 256)
    for kw in (dict(sampling='argmax'), dict(sampling='multinomial', top_k=5)):
        calls.clear()
        weights, samples = _generate(monkeypatch, False, model.decoder, z, **kw)
        assert calls == {'arvae_tick_free_run_wide': 1}, (kw, calls)
        assert tuple(samples.shape) == (5, 24) and bool(torch.isfinite(weights).all())
    calls.clear()
    _generate(monkeypatch, True, model.decoder, z, sampling='argmax')
    assert calls == {'arvae_row_argmax': 24}, calls             # the tick-by-tick pass stays what it was


def test_a_captured_graph_holds_the_free_running_call(dev, monkeypatch):
    """HIP-graph replay of a 256 / 256 model's free-running forward + backward (arvae_amd.graphed, dropout 0, the decoder's coin pinned
    to free running) against the eager step, on other data than it was captured on: the call neither allocates nor synchronises nor
    reads back, so the replay gives a bit-identical loss and gradient arena (test_a_captured_graph_holds_the_wide_calls' method)"""
    from arvae_amd import _lib
    from arvae_amd.graphed import GraphedStep
    from arvae_amd.measure_vae import MeasureVAE
    monkeypatch.delenv('ARVAE_TICK_STEPWISE', raising=False)
    monkeypatch.delenv('ARVAE_GRU_STEPWISE', raising=False)
    lib = _lib.load()
    real, calls = lib.arvae_tick_free_run_wide, []
    monkeypatch.setattr(lib, 'arvae_tick_free_run_wide', lambda *a: (calls.append(1), real(*a))[1])
    model, trainer = _build(0, lambda ds: MeasureVAE(ds, 10, 2, 2, 256, 0.0, 16, 2, 256, 0.0, False, 'folk'), dev)
    b = 32
    model.encoder.static_eps = torch.from_numpy(syn.normal_noise((b, 16), seed=3)).to(dev)
    score = torch.from_numpy(syn.measure_batch(b, seed=8)).to(dev)
    other = torch.from_numpy(syn.measure_batch(b, seed=9)).to(dev)
    try:
        graphed = GraphedStep(trainer, (other, other))
        model.decoder.teacher_forcing_prob = -1.0
        trainer.zero_grad()
        loss, _ = trainer.loss_and_acc_for_batch((score, score), 0, 1, True)
        loss.backward()
        want_loss, want_grad = float(loss.detach()), trainer.optimizer.grad_arena.clone()
        eager_calls = len(calls)
        assert eager_calls >= 1
        graphed.prob = -1.0
        got_loss, _ = graphed((score, score))
        torch.cuda.synchronize()
        assert float(got_loss) == want_loss
        assert torch.equal(trainer.optimizer.grad_arena, want_grad)
    finally:
        type(model.encoder).static_eps = None
        model.encoder.static_eps = None

"""The streamed-weights beam search at hidden sizes 256 and 512 (ar-vae_amd/csrc/beam_wide.hip through ops.tick_beam_search_wide) on
every case of beam_wide_cases.py.  Needs a real MI355X.

  (a) the selection of every tick is ops.beam_select / _planned / _groups on the logits the call returns, the scores (and log_probs)
      of the tick before and the same `live`, exactly (scores bitwise): both see the same bits, so no gap condition is needed;
  (b) the history backtracks to the sequences, the scores are the last tick's, parents and tokens in range and inside the mask or the
      plan, dead slots at -inf listed last;
  (c) those logits against the float64 CPU decoder carried along the call's own history, held to gru_cases.bar's output bar with the
      fp32 CPU decoder's error on the same history as the yardstick (no new tolerance; every figure printed);
  (d) the same call twice: every output bit-identical; without logits_out: the same histories;
  (e) width 1: the argmax free run of ops.tick_free_run_wide, its logits bit for bit;
  (f) the scratch contract (test_tick_wide_gpu.test_scratch_contract's method)."""
import numpy as np
import pytest
import torch

import beam_wide_cases as bc
import gru_cases as gc
import guarded_alloc as ga
from test_beam_search import backtrack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _on(dev, a):
    return None if a is None else torch.from_numpy(a).to(dev)


def _device_problem(dev, p):
    d = {k: _on(dev, p[k]) for k in ('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1', 'w_out', 'b_out', 'h0', 'gib', 'ptab', 'allow',
                                     'plan')}
    d['weights'] = tuple(d[k] for k in ('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1', 'w_out', 'b_out'))
    return d


def _run(p, d, return_logits=True):
    """-> dict(parents, tokens, hist, seqs, scores[, logp][, logits])"""
    from arvae_amd import ops
    groups = (p['groups'], p['penalty']) if p['form'] == 'groups' else None
    out = ops.tick_beam_search_wide(d['weights'], d['h0'][0], d['h0'][1], d['gib'], d['ptab'], p['batch'], p['beats'], p['tpb'], p['width'],
                                    allow=d['allow'], plan=d['plan'], groups=groups, return_logits=return_logits)
    torch.cuda.synchronize()
    names = ['parents', 'tokens', 'hist', 'seqs', 'scores'] + (['logp'] if groups else []) + (['logits'] if return_logits else [])
    assert len(out) == len(names)
    return dict(zip(names, out))


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and int((_bits(a) != _bits(b)).sum()) == 0


@pytest.mark.parametrize('case', bc.CASES, ids=bc.case_id)
def test_every_case(dev, case):
    from arvae_amd import ops
    name = bc.case_id(case)
    p = bc.problem(*case)
    d = _device_problem(dev, p)
    b, ticks, w, vocab, g = p['batch'], p['ticks'], p['width'], p['vocab'], p['groups']
    got = _run(p, d)
    parents, tokens, hist, seqs, scores, logits = (got[k] for k in ('parents', 'tokens', 'hist', 'seqs', 'scores', 'logits'))
    assert parents.dtype == torch.int32 and tokens.dtype == torch.int64 and seqs.dtype == torch.int64
    assert tuple(parents.shape) == tuple(tokens.shape) == tuple(hist.shape) == (b, ticks, w)
    assert tuple(seqs.shape) == (b, w, ticks) and tuple(scores.shape) == (b, w)
    assert tuple(logits.shape) == (b, ticks, w, vocab) and bool(torch.isfinite(logits).all())

    # (a) every tick's selection is the tick-by-tick entry point's
    prev = torch.zeros(b, w, device=dev)
    logp = torch.zeros(b, w, device=dev)
    for t in range(ticks):
        rows = logits[:, t].reshape(b * w, vocab).contiguous()
        live = 1 if t == 0 else w
        if p['form'] == 'groups':
            par, note, sc, logp = ops.beam_select_groups(rows, prev, logp, min(live, w // g), g, p['penalty'], d['plan'], t, ticks)
        elif p['form'] == 'planned':
            par, note, sc = ops.beam_select_planned(rows, prev, live, d['plan'], t)
        else:
            par, note, sc = ops.beam_select(rows, prev, live, d['allow'])
        assert torch.equal(parents[:, t], par), (name, t, parents[:, t].tolist(), par.tolist())
        assert torch.equal(tokens[:, t], note), (name, t, tokens[:, t].tolist(), note.tolist())
        assert _same(hist[:, t], sc), (name, t, hist[:, t].tolist(), sc.tolist())
        prev = hist[:, t].contiguous()
    if p['form'] == 'groups':
        assert _same(got['logp'], logp), name

    # (b) the backtracking and the ranges
    par_h, tok_h, hist_h = parents.cpu().numpy(), tokens.cpu().numpy(), hist.cpu().numpy()
    np.testing.assert_array_equal(backtrack(par_h, tok_h), seqs.cpu().numpy())
    assert _same(scores, hist[:, -1].contiguous())
    assert par_h.min() >= 0 and par_h.max() < w and tok_h.min() >= 0 and tok_h.max() < vocab
    if p['allow'] is not None:
        assert p['allow'][tok_h].all()
    if p['plan'] is not None:
        assert np.take_along_axis(p['plan'], tok_h, 2).all()    # dead slots included
    gw = w // g
    grouped = hist_h.reshape(b, ticks, g, gw)
    with np.errstate(invalid='ignore'):
        assert not (np.diff(grouped, axis=-1) > 0).any()        # non-increasing within a group: the dead slots (-inf) last
    assert not np.isnan(hist_h).any() and not (hist_h == np.inf).any()
    dead = np.isinf(hist_h)
    if p['plan'] is not None:                                   # (every planned case has more than one beam a group)
        assert dead[:, 0].any()                                 # the forced first tick leaves one candidate a group
        assert (par_h.reshape(b, ticks, g, gw) // gw == np.arange(g)[None, None, :, None]).all()       # parents inside the group
    else:
        assert not dead.any()
    if ticks > 1 and vocab > 2:
        assert np.unique(tok_h).size > 2                        # the notes vary

    # (c) the logits against float64, carried along the call's own history
    ref, cpu = bc.reference_logits(p, par_h, tok_h, np.float64), bc.reference_logits(p, par_h, tok_h, np.float32)
    e_hip, e_cpu = gc.rel(logits, ref), gc.rel(cpu, ref)
    bar = gc.bar('y_logits', e_cpu)
    print(f'{name} y_logits: rel {e_hip:.3e}  rel_cpu {e_cpu:.3e}  rel/rel_cpu {e_hip / max(e_cpu, 1e-300):.2f}  bar {bar:.3e}')
    assert e_cpu <= gc.REL_CPU_MAX, (name, 'the fp32 CPU yardstick is further than 1e-6 from float64', e_cpu)
    assert e_hip <= bar, (name, e_hip, bar)

    # (d) the same call twice; without logits_out
    again = _run(p, d)
    assert all(_same(again[k], got[k]) for k in got), name
    bare = _run(p, d, return_logits=False)
    assert 'logits' not in bare and all(_same(bare[k], got[k]) for k in bare), name


def test_width_one_is_the_argmax_free_run(dev):
    """(e): the recurrence and the logits are the tile's, bit for bit"""
    from arvae_amd import ops
    case = (256, 40, 2, 1, 1, 'plain')
    assert case in bc.CASES
    p = bc.problem(*case)
    d = _device_problem(dev, p)
    got = _run(p, d)
    tokens, logits = ops.tick_free_run_wide(d['weights'], d['h0'][0], d['h0'][1], d['gib'], d['ptab'], p['batch'], p['beats'], p['tpb'],
                                            return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(got['seqs'][:, 0], tokens) and torch.equal(got['tokens'][:, :, 0], tokens)
    assert _same(got['logits'][:, :, 0].contiguous(), logits)
    assert int(tokens.unique().numel()) == 2 and int(got['parents'].abs().max()) == 0


SCRATCH_CASES = [(512, 7, 35, 8, 4, 'groups'), (256, 21, 128, 3, 1, 'plain')]


@pytest.mark.parametrize('case', SCRATCH_CASES, ids=bc.case_id)
def test_scratch_contract(dev, monkeypatch, case):
    """(f): one call with every torch.empty of ops guarded and poisoned, 0xFF and then 0x7E: both guard bands of every allocation
    intact -- the workspace's among them --, nothing passed the proxy by, every output bit-identical to the plain run"""
    from arvae_amd import ops
    assert case in bc.CASES
    p = bc.problem(*case)
    d = _device_problem(dev, p)
    plain = _run(p, d)
    for fill in (ga.FILL_NAN, ga.FILL_BIG):
        with monkeypatch.context() as m:
            proxy = ga.GuardedTorch(fill).install(m, ops)
            got = _run(p, d)
        proxy.check_bands()
        assert proxy.passed_through == [] and proxy.records
        # the five outputs (six when grouped), the logits and the workspace
        assert sum('tick_beam_search_wide' in rec.site for rec in proxy.records) >= len(plain) + 1, proxy.by_site()
        assert all(_same(got[k], plain[k]) for k in plain), fill

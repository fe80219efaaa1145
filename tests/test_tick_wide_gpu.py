"""The streamed-weights free-running tick decoder at hidden sizes 256 and 512 (ar-vae_amd/csrc/tick_wide.hip through
ops.tick_free_run_wide) on every case of tick_wide_cases.py.  Needs a real MI355X.

  (a) the pick of every (row, tick) is the row entry point's pick on the logits the call returns, exactly, no row left out: both see
      the same bits, so no gap condition is needed;
  (b) those logits against the float64 CPU decoder fed the kernel's own tokens, held to gru_cases.bar's output bar with the fp32 CPU
      decoder's error on the same tokens as the yardstick (no new tolerance; every figure printed);
  (c) the same call twice: tokens and logits bit-identical;
  (d) without logits_out: the same tokens;
  (e) the scratch contract (test_measure_wide_gpu.test_scratch_contract's method)."""
import numpy as np
import pytest
import torch

import gru_cases as gc
import guarded_alloc as ga
import tick_wide_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _on(dev, a):
    return None if a is None else torch.from_numpy(a).to(dev)


def _device_problem(dev, p):
    d = {k: _on(dev, p[k]) for k in ('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1', 'w_out', 'b_out', 'h0', 'gib', 'ptab', 'mask',
                                     'uniforms', 'allow', 'plan')}
    d['weights'] = tuple(d[k] for k in ('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1', 'w_out', 'b_out'))
    return d


def _run(p, d, return_logits=True):
    from arvae_amd import ops
    flt = None
    if p['form'] == 'filtered':
        flt = (p['top_k'], p['top_p'], d['allow'])
    elif p['plan'] is not None:
        flt = (p['top_k'], p['top_p'])
    out = ops.tick_free_run_wide(d['weights'], d['h0'][0], d['h0'][1], d['gib'], d['ptab'], p['batch'], p['beats'], p['tpb'], mask=d['mask'],
                                 keep_scale=p['keep_scale'], uniforms=d['uniforms'], temperature=p['temperature'], filter=flt,
                                 plan=d['plan'], return_logits=return_logits)
    torch.cuda.synchronize()
    return out


def _row_pick(p, d, logits, t):
    """tick t's pick by the existing row entry point of the case's form, on the call's own logits"""
    from arvae_amd import ops
    w = logits[:, t].contiguous()
    if p['form'] == 'argmax':
        return ops.row_argmax(w)
    u = d['uniforms'][:, t].contiguous()
    if p['form'] == 'multinomial':
        return ops.row_sample(w, u, p['temperature'])
    if p['form'] == 'filtered':
        return ops.row_sample_filtered(w, u, p['temperature'], p['top_k'], p['top_p'], d['allow'])
    return ops.row_sample_planned(w, u, d['plan'], t, p['temperature'], p['top_k'], p['top_p'])


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize('case', tc.CASES, ids=tc.case_id)
def test_every_case(dev, case):
    name = tc.case_id(case)
    p = tc.problem(*case)
    d = _device_problem(dev, p)
    tokens, logits = _run(p, d)
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (p['batch'], p['ticks'])
    assert tuple(logits.shape) == (p['batch'], p['ticks'], p['vocab']) and bool(torch.isfinite(logits).all())
    assert int(tokens.min()) >= 0 and int(tokens.max()) < p['vocab']

    # (a) every pick is the row entry point's
    for t in range(p['ticks']):
        want = _row_pick(p, d, logits, t)
        assert torch.equal(tokens[:, t], want), (name, t, tokens[:, t].tolist(), want.tolist())
    if p['ticks'] > 1:
        assert int(tokens.unique().numel()) > 1                 # the picks vary
    if p['plan'] is not None:                                   # inside the plan; the row and tick with no allowed note: note 0
        allowed = torch.gather(d['plan'], 2, tokens[:, :, None])[:, :, 0] != 0
        empty = d['plan'].sum(-1) == 0
        assert int(empty.sum()) == 1 and bool((allowed | empty).all()) and bool((tokens[empty] == 0).all())
    if p['form'] == 'filtered':
        assert bool((d['allow'][tokens] != 0).all())

    # (b) the logits against float64, fed the kernel's own tokens
    fed = tokens.cpu().numpy()
    ref, cpu = tc.reference_logits(p, fed, np.float64), tc.reference_logits(p, fed, np.float32)
    e_hip, e_cpu = gc.rel(logits, ref), gc.rel(cpu, ref)
    bar = gc.bar('y_logits', e_cpu)
    print(f'{name} y_logits: rel {e_hip:.3e}  rel_cpu {e_cpu:.3e}  rel/rel_cpu {e_hip / max(e_cpu, 1e-300):.2f}  bar {bar:.3e}')
    assert e_cpu <= gc.REL_CPU_MAX, (name, 'the fp32 CPU yardstick is further than 1e-6 from float64', e_cpu)
    assert e_hip <= bar, (name, e_hip, bar)

    # (c) the same call twice
    tokens2, logits2 = _run(p, d)
    assert torch.equal(tokens2, tokens) and int((_bits(logits2) != _bits(logits)).sum()) == 0, name

    # (d) without logits_out
    assert torch.equal(_run(p, d, return_logits=False), tokens), name


SCRATCH_CASES = [(512, 37, 70, 4, 6, 'filtered', False), (256, 5, 35, 4, 6, 'multinomial', True)]


@pytest.mark.parametrize('case', SCRATCH_CASES, ids=tc.case_id)
def test_scratch_contract(dev, monkeypatch, case):
    """one call with every torch.empty of ops guarded and poisoned, 0xFF and then 0x7E: both guard bands of every allocation intact --
    the workspace's among them --, nothing passed the proxy by, tokens and logits bit-identical to the plain run"""
    from arvae_amd import ops
    assert case in tc.CASES
    p = tc.problem(*case)
    d = _device_problem(dev, p)
    plain = _run(p, d)
    for fill in (ga.FILL_NAN, ga.FILL_BIG):
        with monkeypatch.context() as m:
            proxy = ga.GuardedTorch(fill).install(m, ops)
            got = _run(p, d)
        proxy.check_bands()
        assert proxy.passed_through == [] and proxy.records
        assert sum('tick_free_run_wide' in rec.site for rec in proxy.records) >= 3, proxy.by_site()     # tokens, logits, workspace
        assert torch.equal(got[0], plain[0]) and int((_bits(got[1]) != _bits(plain[1])).sum()) == 0, fill

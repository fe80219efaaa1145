"""The streamed-weights GRU recurrences at hidden sizes 256 and 512 (ar-vae_amd/csrc/gru_wide.hip) through ops.dense and
ops.gru_sequence against a float64 nn.GRU.  Needs a real MI355X.

Every case of gru_wide_cases.CASES: the outputs, the final states and the gradients of x, h0, weight_ih, bias_ih, weight_hh and
bias_hh of all four directions are held to the bars of gru_cases.bar (outputs 2e-6 .. 3e-6, gradients 2e-5: no new number), each
figure printed.  Without the wide entry points these tests fail with "hidden size 256 is not built".

Further: initial states of 6000 and recurrent weights times 300 stay finite (three-term bf16 operands need no scale) and hold the
unclamped bars, as test_workgroup_state_scale does for the resident-weights kernels; the same call twice is bit-identical (the
partial sums of the four K quarters are added in a fixed order, no atomics)."""
import copy

import numpy as np
import pytest
import torch

import gru_cases as gc
import gru_wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _hip_results(dev, p, nseq=4, variant='plain'):
    """the problem through ops.dense and ops.gru_sequence calls of `nseq` sequences -> the tensors of gru_cases.references"""
    from arvae_amd import ops
    hid, steps, rows, fin_w = p['hid'], p['steps'], p['rows'], gc.FIN
    dirs, leaves, merged = [], [], []
    for k, gru in enumerate(p['layers']):
        prm = {n: v.detach().clone().to(dev).requires_grad_(True) for n, v in gru.named_parameters()}
        const = variant == 'constant_gi'
        xd = (p['x'][k][0] if const else p['x'][k]).to(dev).requires_grad_(True)
        hd = None if variant == 'no_h0' else p['h0'][k].to(dev).requires_grad_(True)
        x2 = xd if const else xd.view(steps * rows, fin_w)
        cat = None
        if variant == 'merged_gi':                             # both directions' projections as one GEMM, read with a row stride
            cat = (torch.cat((prm['weight_ih_l0'], prm['weight_ih_l0_reverse'])).detach().requires_grad_(True),
                   torch.cat((prm['bias_ih_l0'], prm['bias_ih_l0_reverse'])).detach().requires_grad_(True))
            merged.append(ops.dense(x2, cat[0], cat[1], ops.Link.dense(fin_w, 6 * hid), 0).view(steps, rows, 6 * hid))
        for d, suf in enumerate(('', '_reverse')):
            gi = None
            if cat is None:
                gi = ops.dense(x2, prm['weight_ih_l0' + suf], prm['bias_ih_l0' + suf], ops.Link.dense(fin_w, 3 * hid), 0)
                gi = gi if const else gi.view(steps, rows, 3 * hid)
            dirs.append((gi, prm['weight_hh_l0' + suf], prm['bias_hh_l0' + suf], None if hd is None else hd[d], gc.REVERSE[2 * k + d]))
        leaves.append((prm, xd, hd, cat))
    outs, fins = [], []
    for a, b in wc.chunks(nseq):
        mg = None
        if variant == 'merged_gi':
            assert (a % 2, b - a) == (0, 2)
            mg = merged[a // 2]
        o, f = ops.gru_sequence(steps, dirs[a:b], merged_gi=mg)
        assert o.shape == (steps, rows, (b - a) * hid) and f.shape == (rows, (b - a) * hid)
        outs.append(o)
        fins.append(f)
    yd, fin = torch.cat(outs, 2), torch.cat(fins, 1)
    loss = (fin * torch.cat(list(p['gfin']), 1).to(dev)).sum()
    if variant != 'finals_only':
        loss = loss + (yd * torch.cat(list(p['gy']), 2).to(dev)).sum()
    loss.backward()
    out = {}
    for k, (prm, xd, hd, cat) in enumerate(leaves):
        cols = slice(2 * hid * k, 2 * hid * (k + 1))
        out.update({f'y{k}': yd.detach()[:, :, cols], f'hn{k}': fin.detach()[:, cols], f'dx{k}': xd.grad})
        if hd is not None:
            out[f'dh0_{k}'] = hd.grad
        grads = {n: v.grad for n, v in prm.items()}
        if cat is not None:
            grads.update({'weight_ih_l0': cat[0].grad[:3 * hid], 'weight_ih_l0_reverse': cat[0].grad[3 * hid:],
                          'bias_ih_l0': cat[1].grad[:3 * hid], 'bias_ih_l0_reverse': cat[1].grad[3 * hid:]})
        out.update({f'd{n}[{k}]': g for n, g in grads.items()})
    return out


def _hold(case, got, cpu, ref, conditioned=True):
    """the bars of gru_cases.py on every tensor, each figure printed (test_gru_recurrences_float64._hold)"""
    assert set(got) == set(ref) == set(cpu), (case, sorted(set(got) ^ set(ref)))
    figures = {k: (gc.rel(got[k], ref[k]), gc.rel(cpu[k], ref[k])) for k in ref}
    bars = {k: gc.bar(k, e_cpu, clamp=conditioned) for k, (_, e_cpu) in figures.items()}
    for k, (e_hip, e_cpu) in figures.items():
        print(f'{case} {k}: rel {e_hip:.3e}  rel_cpu {e_cpu:.3e}  rel/rel_cpu {e_hip / max(e_cpu, 1e-300):.2f}  bar {bars[k]:.3e}')
    if conditioned:
        slack = {k: e_cpu for k, (_, e_cpu) in figures.items() if gc.yardstick_is_held(k) and not e_cpu <= gc.REL_CPU_MAX}
        assert not slack, (case, 'the fp32 CPU yardstick is further than 1e-6 from float64', slack)
    for k in got:
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (case, k)
    bad = {k: v for k, v in figures.items() if not v[0] <= bars[k]}
    assert not bad, (case, bad)


@pytest.mark.parametrize('case', wc.CASES, ids=wc.case_id)
def test_every_case_vs_float64(dev, case):
    hid, steps, rows, nseq, variant = case
    p = wc.variant_problem(hid, steps, rows, variant)
    ref, cpu = wc.references(hid, steps, rows, variant)
    _hold(wc.case_id(case), _hip_results(dev, p, nseq, variant), cpu, ref)


def test_large_initial_states(dev):
    """H = 256, 69 rows, initial states up to 6000 in three rows: two in the second row tile, one in the ragged last.  Everything is
    finite and the unclamped bars hold (a state of 6000 behind a gate is ill-conditioned in fp32 itself: the bars' 3 x and 5 x
    rel_cpu terms are for that, as in test_workgroup_state_scale)."""
    rows, big = 69, (33, 34, 67)
    assert all(r // 32 == 1 for r in big[:2]) and big[2] // 32 == rows // 32 and rows % 32 == 5
    p = gc.problem(256, 6, rows, 6000.0, big)
    assert float(p['h0'].abs().max()) > 4094.0 and float(np.abs(np.delete(p['h0'].numpy(), big, axis=2)).max()) <= 1.0
    ref, cpu = gc.references(256, 6, rows, 6000.0, big)
    _hold('h0 x 6000', _hip_results(dev, p), cpu, ref, conditioned=False)


def test_large_recurrent_weights(dev):
    """W_hh times 300 at H = 256, 37 rows, THREE steps: finite, with the same unclamped bars.
    Why three steps: a recurrence with weights this large amplifies a rounding error about tenfold per step in float32 itself --
    torch's fp32 CPU layer is 3e-6 .. 4e-5 from float64 after one step, 6e-5 .. 4e-4 after two, 6e-4 .. 4e-3 after three and
    0.19 .. 1.1 after six (every tensor wrong in its leading digit: the multiple of such a figure holds nothing).  Three steps run
    the large weights through three forward GEMMs, two backward ones and the tail launch, and leave a yardstick that means something:
    the test asserts first that it is within 1e-2 of float64 on every tensor."""
    p = dict(gc.problem(256, 3, 37))
    p['layers'] = [copy.deepcopy(g) for g in p['layers']]
    with torch.no_grad():
        for g in p['layers']:
            g.weight_hh_l0.mul_(300.0)
            g.weight_hh_l0_reverse.mul_(300.0)
        assert float(p['layers'][0].weight_hh_l0.abs().max()) > 15.0          # 300 / sqrt(256) = 18.75 at most
    ref, cpu = gc._torch_results(p, torch.float64), gc._torch_results(p, torch.float32)
    loose = {k: gc.rel(cpu[k], ref[k]) for k in ref if not gc.rel(cpu[k], ref[k]) <= 1e-2}
    assert not loose, ('fp32 itself cannot be held on this problem', loose)
    _hold('W_hh x 300', _hip_results(dev, p), cpu, ref, conditioned=False)


def test_same_call_twice_is_bit_identical(dev):
    p = gc.problem(512, 6, 37)
    a, b = _hip_results(dev, p), _hip_results(dev, p)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k

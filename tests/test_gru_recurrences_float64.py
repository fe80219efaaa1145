"""The whole-sequence GRU recurrences (ar-vae_amd/csrc/gru_seq.hip) at every hidden size and every row width, through ops.dense and
ops.gru_sequence: bit for bit against themselves at another row width, and against a float64 nn.GRU.  Needs a real MI355X.

The host picks the batch rows per workgroup RW from the row count, the sequences in the launch and the CU count (gru_rows_per_wg,
gru_common.h; restated in gru_cases.rows_per_wg).  Every test takes the device's CU count, derives its row counts from it
(gru_cases.rows_for) and asserts through the restatement that each launch lands on the width it is named for.

Case -> kernel instantiation at 256 CUs (confirmed once with a kernel trace of this file: all eighteen names below appear, and no
other gru_seq kernel):

  rows x sequences in the launch                            forward                          backward
  21 x 4, and every chunk of <= 4 * (CUs // nseq) rows      gru_seq_fwd_h2_kernel<H, 4>      gru_seq_bwd_h2_kernel<H, 4>
  261 x 4 (517 x 2, 345 x 3)                                gru_seq_fwd_h2_kernel<H, 8>      gru_seq_bwd_h2_kernel<H, 8>
  517 x 4 (1029 x 2, 2053 x 1)                              gru_seq_fwd_h2_kernel<H, 16>     gru_seq_bwd_h2_kernel<H, 16>
  for H = 32, 64 and 128 each: nine forward and nine backward instantiations.

  test_rows_do_not_depend_on_the_row_width[H-RW]     <H, 8> or <H, 16> whole, <H, 4> in chunks (256 + 5, 256 + 256 + 5 rows)
  test_variants_do_not_depend_on_the_row_width       no_h0 <32, 16>; finals_only <64, 16>; constant_gi <128, 8>; merged_gi <64, 8>
                                                     with two sequences; one_sequence <128, 16>; three_sequences <32, 8>; each
                                                     against <H, 4> chunks
  test_every_instantiation_vs_float64[H-RW-T]        <H, RW> forward and backward, T = 6 for all nine, T = 24 at RW 8
  test_workgroup_state_scale[RW]                     <64, RW> with initial states of 6000 in three rows, and <64, 4> chunks

What the unrun widths execute that RW 4 at H = 128 never does: the loops that issue the memory traffic of the rows left over once
the k-step groups are used up (H = 32 at RW 8 and 16, H = 64 at RW 16), the spread_pairs lane mapping of RW 8 (gru_lrow<2>,
gru_arow<2>), and the padded slots of the backward kernel's row maxima at H = 32.

Why rows are comparable bit for bit: each batch row is an independent recurrence.  A row of a 16 x 16 x 32 MFMA result depends on
that row of the A operand only; W_hh's scale is per wave, the backward operand's scale per row and step, and the one
workgroup-wide quantity, the state's scale pow2_for(max(1, max |h0|)), is the same constant in every workgroup while |h0| <= 1."""
import numpy as np
import pytest
import torch

from gru_cases import (CASES, FIN, NSEQ, REL_CPU_MAX, REVERSE, bar, chunk_rows, problem, references, rel, rows_for, rows_per_wg,
                       yardstick_is_held)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows(rw, nseq, cus):
    """the table's row count for a width, held to that width on THIS device: never the wrong kernel under the right name"""
    rows = rows_for(rw, nseq, cus)
    assert rows_per_wg(rows, nseq, cus) == rw and rows % rw != 0, \
        f'{rows} rows x {nseq} sequences on {cus} CUs run {rows_per_wg(rows, nseq, cus)} rows per workgroup, not {rw}'
    return rows


# ---------------------------------------------------------------- a. row widths are the same arithmetic, bit for bit
def _bit_problem(hid, steps, rows, nseq, seed, const_gi=False, big_rows=(), h_big=1.0):
    """input projections fed directly (leaf tensors: their gradient is the kernel's dgi), recurrent weights drawn as nn.GRU draws
    them, initial states uniform in [-1, 1] (rows `big_rows` times `h_big`), gradients for the outputs and the final states"""
    rs = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(hid)
    h0 = rs.uniform(-1.0, 1.0, (nseq, rows, hid))
    for r in big_rows:
        h0[:, r] *= h_big
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))             # noqa: E731
    return dict(hid=hid, steps=steps, rows=rows, nseq=nseq,
                gi=f32(rs.standard_normal((nseq, rows, 3 * hid) if const_gi else (nseq, steps, rows, 3 * hid))),
                w_hh=f32(rs.uniform(-k, k, (nseq, 3 * hid, hid))), b_hh=f32(rs.uniform(-k, k, (nseq, 3 * hid))), h0=f32(h0),
                d_out=f32(rs.standard_normal((steps, rows, nseq * hid))), d_fin=f32(rs.standard_normal((rows, nseq * hid))))


def _run_rows(dev, q, a, b, use_h0=True, use_d_out=True, merged=False):
    """rows [a, b) of the problem as one launch -> name -> tensor, the batch rows in dimension -2 of every one"""
    from arvae_amd import ops
    nseq, steps = q['nseq'], q['steps']
    reverse = REVERSE[:nseq]
    gis = [q['gi'][s][..., a:b, :].contiguous().to(dev) for s in range(nseq)]
    h0s = [q['h0'][s][a:b].contiguous().to(dev).requires_grad_(True) if use_h0 else None for s in range(nseq)]
    whs, bhs = [q['w_hh'][s].to(dev) for s in range(nseq)], [q['b_hh'][s].to(dev) for s in range(nseq)]
    if merged:
        leaves = [torch.cat(gis, -1).requires_grad_(True)]
        dirs = [(None, whs[s], bhs[s], h0s[s], reverse[s]) for s in range(nseq)]
        out, fin = ops.gru_sequence(steps, dirs, merged_gi=leaves[0])
    else:
        leaves = [g.requires_grad_(True) for g in gis]
        out, fin = ops.gru_sequence(steps, [(leaves[s], whs[s], bhs[s], h0s[s], reverse[s]) for s in range(nseq)])
    loss = (fin * q['d_fin'][a:b].to(dev)).sum()
    if use_d_out:
        loss = loss + (out * q['d_out'][:, a:b].contiguous().to(dev)).sum()
    loss.backward()
    got = {'out': out.detach(), 'fin': fin.detach()}
    got.update({f'dgi{i}': g.grad for i, g in enumerate(leaves)})
    if use_h0:
        got.update({f'dh0_{s}': h.grad for s, h in enumerate(h0s)})
    assert all(v is not None and v.shape[-2] == b - a for v in got.values())
    return got


def _whole_and_chunks(dev, q, rw, cus, chunk=None, **how):
    """the problem as one launch at `rw` rows per workgroup, and again as chunks of rows that run at 4"""
    rows, nseq = q['rows'], q['nseq']
    assert rows_per_wg(rows, nseq, cus) == rw, (rows, nseq, cus, rw)
    chunk = chunk_rows(nseq, cus) if chunk is None else chunk
    whole = _run_rows(dev, q, 0, rows, **how)
    parts = []
    for a in range(0, rows, chunk):
        b = min(a + chunk, rows)
        assert rows_per_wg(b - a, nseq, cus) == 4, (b - a, nseq, cus)
        parts.append(_run_rows(dev, q, a, b, **how))
    return whole, {k: torch.cat([p[k] for p in parts], -2) for k in whole}


def _assert_same_rows(case, whole, chunks, keep=None):
    bad = []
    for k in whole:
        w, c = (v if keep is None else v[..., keep, :] for v in (whole[k], chunks[k]))
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(c).all()), (case, k)
        if not torch.equal(w, c):
            rows = torch.nonzero((w != c).reshape(-1, *w.shape[-2:]).any(0).any(-1)).flatten().tolist()
            bad.append((k, len(rows), rows[:8], float((w - c).abs().max())))
    assert not bad, (case, bad)


@pytest.mark.parametrize('rw', [8, 16])
@pytest.mark.parametrize('hid', [32, 64, 128])
def test_rows_do_not_depend_on_the_row_width(dev, cus, hid, rw):
    """four sequences (reverse flags F, T, F, T) of 6 steps over 261 rows (RW 8) or 517 rows (RW 16), and the same rows again in
    chunks of at most 4 * (CUs // 4) rows (RW 4): outputs, final states, the input projections' gradient (the kernel's dgi) and the
    initial states' gradient are equal bit for bit in every row -- the ragged last workgroup's five rows among them.
    (W_hh's and b_hh's gradients come out of a dense launch over a different row count: test_every_instantiation_vs_float64)"""
    q = _bit_problem(hid, 6, _rows(rw, NSEQ, cus), NSEQ, seed=100 * hid + rw)
    whole, chunks = _whole_and_chunks(dev, q, rw, cus)
    _assert_same_rows(f'H{hid} RW{rw}', whole, chunks)


VARIANTS = {   # name: (hidden, rows per workgroup, sequences, how)
    'no_h0':           (32, 16, 4, dict(use_h0=False)),                   # the initial state is null: zeros, and no dh0
    'finals_only':     (64, 16, 4, dict(use_d_out=False)),                # dh_all null: only the final states carry a gradient
    'constant_gi':     (128, 8, 4, dict(const_gi=True)),                  # gi_tstride 0: one projection for every step
    'merged_gi':       (64, 8, 2, dict(merged=True)),                     # one (T, R, 2 * 3H) projection read with a row stride
    'one_sequence':    (128, 16, 1, dict()),
    'three_sequences': (32, 8, 3, dict()),
}


@pytest.mark.parametrize('name', list(VARIANTS))
def test_variants_do_not_depend_on_the_row_width(dev, cus, name):
    """the launch's other forms, each at RW 8 or 16 against its RW 4 chunks, bit for bit as above.  constant_gi: the projection's
    gradient is the sum over the steps of the kernel's dgi (one torch sum over the step dimension, the same order for any row
    count)."""
    hid, rw, nseq, how = VARIANTS[name]
    how = dict(how)
    q = _bit_problem(hid, 6, _rows(rw, nseq, cus), nseq, seed=7 * hid + rw + nseq, const_gi=how.pop('const_gi', False))
    whole, chunks = _whole_and_chunks(dev, q, rw, cus, **how)
    assert ('dh0_0' in whole) == (name != 'no_h0') and len([k for k in whole if k.startswith('dgi')]) == (1 if name == 'merged_gi' else nseq)
    _assert_same_rows(name, whole, chunks)


# ---------------------------------------------------------------- b. every instantiation against float64
def _hip_results(dev, p):
    """problem(...) through ops.dense and ONE ops.gru_sequence launch of four sequences -> the tensors of gru_cases.references"""
    from arvae_amd import ops
    hid, steps, rows = p['hid'], p['steps'], p['rows']
    dirs, leaves = [], []
    for k, gru in enumerate(p['layers']):
        prm = {n: v.detach().clone().to(dev).requires_grad_(True) for n, v in gru.named_parameters()}
        xd, hd = p['x'][k].to(dev).requires_grad_(True), p['h0'][k].to(dev).requires_grad_(True)
        for d, suf in enumerate(('', '_reverse')):
            gi = ops.dense(xd.view(steps * rows, FIN), prm['weight_ih_l0' + suf], prm['bias_ih_l0' + suf],
                           ops.Link.dense(FIN, 3 * hid), 0).view(steps, rows, 3 * hid)
            dirs.append((gi, prm['weight_hh_l0' + suf], prm['bias_hh_l0' + suf], hd[d], REVERSE[2 * k + d]))
        leaves.append((prm, xd, hd))
    yd, fin = ops.gru_sequence(steps, dirs)
    ((yd * torch.cat(list(p['gy']), 2).to(dev)).sum() + (fin * torch.cat(list(p['gfin']), 1).to(dev)).sum()).backward()
    out = {}
    for k, (prm, xd, hd) in enumerate(leaves):
        cols = slice(2 * hid * k, 2 * hid * (k + 1))
        out.update({f'y{k}': yd.detach()[:, :, cols], f'hn{k}': fin.detach()[:, cols], f'dx{k}': xd.grad, f'dh0_{k}': hd.grad})
        out.update({f'd{n}[{k}]': v.grad for n, v in prm.items()})
    return out


def _hold(case, got, cpu, ref, conditioned=True):
    """the bars of gru_cases.py on every tensor, each figure printed; first the yardstick's own distance to float64 (conditioned:
    within 1e-6 wherever it does not hang on the host's BLAS, and clamped there in every bar)"""
    assert set(got) == set(ref) == set(cpu), case
    figures = {k: (rel(got[k], ref[k]), rel(cpu[k], ref[k])) for k in ref}
    bars = {k: bar(k, e_cpu, clamp=conditioned) for k, (_, e_cpu) in figures.items()}
    for k, (e_hip, e_cpu) in figures.items():
        print(f'{case} {k}: rel {e_hip:.3e}  rel_cpu {e_cpu:.3e}  rel/rel_cpu {e_hip / max(e_cpu, 1e-300):.2f}  bar {bars[k]:.3e}')
    if conditioned:
        slack = {k: e_cpu for k, (_, e_cpu) in figures.items() if yardstick_is_held(k) and not e_cpu <= REL_CPU_MAX}
        assert not slack, (case, 'the fp32 CPU yardstick is further than 1e-6 from float64', slack)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (case, k)
    bad = {k: v for k, v in figures.items() if not v[0] <= bars[k]}
    assert not bad, (case, bad)


@pytest.mark.parametrize('hid,rw,steps', CASES, ids=[f'H{h}-RW{w}-T{t}' for h, w, t in CASES])
def test_every_instantiation_vs_float64(dev, cus, hid, rw, steps):
    """Two bidirectional GRU layers with their own parameters as ONE launch of four sequences, input width 10 through ops.dense,
    initial states in [-1, 1], gradients into the outputs and the final states: the outputs, the final states and the gradients of
    x, h0, weight_ih, bias_ih, weight_hh and bias_hh of every sequence against a float64 nn.GRU, with torch's fp32 CPU nn.GRU as
    the yardstick (bars: gru_cases.py; the yardstick itself within 1e-6 of float64, asserted first, and counted for no more in a bar).
    What the bar sees: a lost cross product of the two-term split is 2^-11 of gh, about 1e-4 of the output -- fifty times the
    outputs' bar (the model of the split and of each lost term: test_two_term_arithmetic.py).  Measured once on a scratch build
    with l h' removed from the forward recurrence's products: all twelve cases fail, outputs and final states at 3.9e-5 to 1.4e-4
    (bar 2e-6) and gradients up to 6.4e-5 (bar 2e-5), where the kernels as they stand give 1.4e-7 to 2.8e-7 and 0.8e-7 to 3.5e-7 --
    at most 2.3 and 2.5 times the fp32 CPU layer's own distance."""
    rows = _rows(rw, NSEQ, cus)
    p = problem(hid, steps, rows)
    ref, cpu = references(hid, steps, rows)
    _hold(f'H{hid} RW{rw} T{steps}', _hip_results(dev, p), cpu, ref)


# ---------------------------------------------------------------- c. the workgroup-wide state scale
@pytest.mark.parametrize('rw', [4, 8, 16])
def test_workgroup_state_scale(dev, cus, rw):
    """H = 64 with initial states up to 6000 in three rows (two in the second workgroup, one in the ragged last one) and within
    [-1, 1] everywhere else.  The state's fp16 scale is the workgroup's: pow2_for(max(1, max |h0|)) over the rows it owns.
    (1) Everything is finite and the bars of test_every_instantiation_vs_float64 hold.  The yardstick's own 1e-6 condition is neither
    asserted nor applied here: a state of 6000 behind a gate is ill-conditioned in fp32 itself (the fp32 CPU layer is up to 6e-2 from float64
    on these tensors), which is what the bars' 3 x and 5 x rel_cpu terms are for, as in test_fp16_recurrences_scale_themselves.
    (2) The rows of workgroups WITHOUT a large initial state keep the constant scale, so they are still equal bit for bit to the
    same rows run at RW 4 (in chunks; for the RW 4 case chunks of 12 rows, which keeps each workgroup's four rows together)."""
    rows = _rows(rw, NSEQ, cus)
    big = (rw + 1, rw + 2, rows - 2)
    p = problem(64, 6, rows, 6000.0, big)
    assert float(p['h0'].abs().max()) > 4094.0 and float(np.abs(np.delete(p['h0'].numpy(), big, axis=2)).max()) <= 1.0
    ref, cpu = references(64, 6, rows, 6000.0, big)
    _hold(f'h0 x 6000, RW{rw}', _hip_results(dev, p), cpu, ref, conditioned=False)
    q = _bit_problem(64, 6, rows, NSEQ, seed=640 + rw, big_rows=big, h_big=6000.0)
    whole, chunks = _whole_and_chunks(dev, q, rw, cus, chunk=12 if rw == 4 else None)
    clean = torch.tensor([r for r in range(rows) if all(r // rw != b // rw for b in big)], device=dev)
    assert rows - 3 * rw <= len(clean) < rows - 3
    _assert_same_rows(f'h0 x 6000, RW{rw}', whole, chunks, keep=clean)

"""Case table, bars and reference problems of the float64 tests of the whole-sequence GRU recurrences (ar-vae_amd/csrc/gru_seq.hip:
gru_seq_fwd_h2_kernel<H, RW> and gru_seq_bwd_h2_kernel<H, RW>, H in 32, 64, 128 and RW in 4, 8, 16 batch rows per workgroup), shared
by the CPU test of the table itself (test_gru_cases.py) and the GPU test (test_gru_recurrences_float64.py).
No test in here: the tables and the torch layers only.

The bars are those of test_fp16_recurrences_scale_themselves (test_hip_parity.py), no new number:
  outputs and final states   rel <= max(OUT_FLOOR, OUT_R * rel_cpu)      OUT_FLOOR = 2e-6, OUT_R = 3
  every gradient             rel <= max(GRAD_FLOOR, GRAD_R * rel_cpu)    GRAD_FLOOR = 2e-5, GRAD_R = 5
  rel       largest absolute difference to the float64 nn.GRU result / that result's largest magnitude
  rel_cpu   the same figure of torch's fp32 CPU nn.GRU on the same tensors
and, so that the yardstick cannot inflate a bar, rel_cpu counts for at most REL_CPU_MAX = 1e-6 in a bar (bar() clamps it): no
output's bar is above 3e-6 and every gradient's bar is its floor, on any host.
The yardstick is torch on the host's CPU and not the same everywhere.  On one host it is within 1e-6 of float64 on every tensor of
every case (0.7e-7 to 6.1e-7); on another the input projection's weight gradient -- one fp32 GEMM of the host's BLAS over
steps x rows = 3102 to 6264 terms -- is 1.0e-6 to 2.7e-6 away and every other tensor as before.  So both tests assert
rel_cpu <= REL_CPU_MAX on every tensor except those (HOST_BLAS_SUMS), for which the clamp alone keeps the bar down."""
import functools

import numpy as np
import torch

OUT_FLOOR, OUT_R = 2.0e-6, 3.0
GRAD_FLOOR, GRAD_R = 2.0e-5, 5.0
REL_CPU_MAX = 1.0e-6

HIDDEN = (32, 64, 128)
WIDTHS = (4, 8, 16)
NSEQ = 4                                   # GRU_SEQ_MAX: two bidirectional layers with their own parameters in one launch
REVERSE = (False, True, False, True)
FIN = 10                                   # input width (the note embedding's)
CUS = 256                                  # the MI355X; the GPU test takes the device's own count

# (hidden, rows per workgroup, steps): every instantiation at the tick RNN's 6 steps, and the encoder's 24 steps once per hidden size
CASES = [(hid, rw, 6) for hid in HIDDEN for rw in WIDTHS] + [(hid, 8, 24) for hid in HIDDEN]


def rows_per_wg(rows, nseq, cus):
    """gru_rows_per_wg (gru_common.h): the smallest of 4 and 8 whose workgroups are all on the chip at once, else 16"""
    for rw in (4, 8):
        if -(-rows // rw) * nseq <= cus:
            return rw
    return 16


def rows_for(rw, nseq, cus):
    """a ragged row count that selects `rw` rows per workgroup for `nseq` sequences on `cus` CUs: 5 rows beyond what the next
    narrower width can place (261 and 517 at 256 CUs and four sequences: the last workgroup owns 5 live rows of 8 or 16);
    21 rows = five workgroups and one row for the narrowest"""
    return {4: 21, 8: 4 * (cus // nseq) + 5, 16: 8 * (cus // nseq) + 5}[rw]


def chunk_rows(nseq, cus):
    """the most rows a launch of `nseq` sequences runs at 4 rows per workgroup"""
    return 4 * (cus // nseq)


def rel(got, want):
    got, want = (np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, np.float64) for v in (got, want))
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)


HOST_BLAS_SUMS = ('dweight_ih',)           # tensor names (prefixes) whose yardstick is a long reduction of the host's BLAS


def yardstick_is_held(name):
    return not name.startswith(HOST_BLAS_SUMS)


def bar(name, rel_cpu, clamp=True):
    """the bar of tensor `name`: 'y*' and 'hn*' are outputs and final states, everything else is a gradient.  clamp=False only for
    deliberately ill-conditioned problems, where the fp32 yardstick's own error is the point"""
    if clamp:
        rel_cpu = min(rel_cpu, REL_CPU_MAX)
    if name.startswith(('y', 'hn')):
        return max(OUT_FLOOR, OUT_R * rel_cpu)
    return max(GRAD_FLOOR, GRAD_R * rel_cpu)


@functools.lru_cache(maxsize=None)
def problem(hid, steps, rows, h_big=0.0, big_rows=()):
    """two bidirectional fp32 nn.GRU layers (four independent parameter sets, reverse flags F, T, F, T) and their tensors: inputs of
    width 10, initial states uniform in [-1, 1] (rows `big_rows` times `h_big`), gradients of the outputs and of the final states.
    The returned tensors are shared between tests: nobody writes to them."""
    torch.manual_seed(1000 * hid + steps)
    rs = np.random.RandomState(hid + steps + rows)
    layers = [torch.nn.GRU(FIN, hid, 1, bidirectional=True) for _ in range(2)]
    h0 = rs.uniform(-1.0, 1.0, (2, 2, rows, hid))
    for r in big_rows:
        h0[:, :, r] *= h_big
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))             # noqa: E731
    return dict(hid=hid, steps=steps, rows=rows, layers=layers, x=f32(rs.standard_normal((2, steps, rows, FIN))), h0=f32(h0),
                gy=f32(rs.standard_normal((2, steps, rows, 2 * hid))), gfin=f32(rs.standard_normal((2, rows, 2 * hid))))


def _torch_results(p, dtype):
    out = {}
    for k, gru in enumerate(p['layers']):
        g = torch.nn.GRU(FIN, p['hid'], 1, bidirectional=True).to(dtype)
        g.load_state_dict({n: v.to(dtype) for n, v in gru.state_dict().items()})
        x, h0 = p['x'][k].to(dtype).requires_grad_(True), p['h0'][k].to(dtype).requires_grad_(True)
        y, hn = g(x, h0)
        ((y * p['gy'][k].to(dtype)).sum() + (torch.cat((hn[0], hn[1]), 1) * p['gfin'][k].to(dtype)).sum()).backward()
        out.update({f'y{k}': y.detach(), f'hn{k}': torch.cat((hn[0], hn[1]), 1).detach(), f'dx{k}': x.grad, f'dh0_{k}': h0.grad})
        out.update({f'd{n}[{k}]': v.grad for n, v in g.named_parameters()})
    return out


@functools.lru_cache(maxsize=None)
def references(hid, steps, rows, h_big=0.0, big_rows=()):
    """(float64 results, fp32 CPU results) of problem(...): name -> tensor, computed once per process"""
    p = problem(hid, steps, rows, h_big, big_rows)
    return _torch_results(p, torch.float64), _torch_results(p, torch.float32)

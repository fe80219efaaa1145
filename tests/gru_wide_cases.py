"""Case table and reference problems of the tests of the streamed-weights GRU recurrences at hidden sizes 256 and 512
(ar-vae_amd/csrc/gru_wide.hip: gru_wide_fwd_step_kernel<H> and gru_wide_bwd_step_kernel<H>, one launch per time step), shared by the
CPU test of the table itself (test_gru_wide_cases.py) and the GPU test (test_gru_wide_float64.py).  No test in here.

Bars, the torch layers and the float64 / fp32 CPU results come from gru_cases.py; nothing here adds a number.

A case is (hidden, steps, rows, nseq, variant):
  rows     5 (fewer than any row tile) and, for every row-tile height the kernels are instantiated with (ROW_TILES), a count that is
           5 modulo that height with at least one full tile: the ragged last tile and a full one both run
  steps    1 (the first processed step is also the last), 6 (the tick RNN) and 24 (the encoder)
  nseq     sequences per library call, 1 to 4: the problem's four directions (reverse flags F, T, F, T) go through
           ops.gru_sequence in chunks of nseq
  variant  the forms of VARIANTS in test_gru_recurrences_float64.py"""
import functools

import torch

import gru_cases as gc

HIDDEN = (256, 512)
ROW_TILES = (32,)                          # GWT_RT of gru_wide_tile.h: every row-tile height a kernel is instantiated with
ROWS = (5, 37, 69)                         # 37 = 32 + 5, 69 = 2 * 32 + 5
STEPS = (1, 6, 24)
VARIANT_NAMES = ('plain', 'no_h0', 'finals_only', 'constant_gi', 'merged_gi')

CASES = [
    (256, 6, 37, 4, 'plain'), (512, 6, 37, 4, 'plain'),
    (256, 24, 69, 2, 'plain'), (512, 24, 37, 3, 'plain'),
    (256, 1, 5, 1, 'plain'), (512, 1, 37, 4, 'plain'), (512, 6, 5, 1, 'plain'),
    (256, 6, 37, 4, 'no_h0'),              # the initial state is null: zeros, no GEMM in the first step, no dh0 (no tail launch)
    (512, 6, 5, 4, 'finals_only'),         # dh_all null: only the final states carry a gradient
    (256, 6, 69, 4, 'constant_gi'),        # gi_tstride 0: one projection for every step
    (512, 6, 37, 2, 'merged_gi'),          # one (T, R, 2 * 3H) projection read and written with a row stride
]


def case_id(case):
    hid, steps, rows, nseq, variant = case
    return f'H{hid}-T{steps}-R{rows}-N{nseq}-{variant}'


def chunks(nseq):
    """the four directions of a problem as library calls of `nseq` sequences: [(first, last + 1), ...]"""
    return [(a, min(a + nseq, gc.NSEQ)) for a in range(0, gc.NSEQ, nseq)]


def variant_problem(hid, steps, rows, variant):
    """gru_cases.problem(...) as the variant sees it (shared tensors are replaced, never written)"""
    p = dict(gc.problem(hid, steps, rows))
    if variant == 'no_h0':
        p['h0'] = torch.zeros_like(p['h0'])
    elif variant == 'finals_only':
        p['gy'] = torch.zeros_like(p['gy'])
    elif variant == 'constant_gi':
        p['x'] = p['x'][:, :1].expand(-1, steps, -1, -1).contiguous()
    return p


@functools.lru_cache(maxsize=None)
def references(hid, steps, rows, variant):
    """(float64 results, fp32 CPU results) of the variant's problem, name -> tensor as gru_cases.references; computed once.
    no_h0: no gradient of the initial state; constant_gi: the input's gradient summed over the steps (one input row per batch row)"""
    if variant in ('plain', 'merged_gi'):
        return gc.references(hid, steps, rows)
    p = variant_problem(hid, steps, rows, variant)
    out = []
    for dtype in (torch.float64, torch.float32):
        r = gc._torch_results(p, dtype)
        if variant == 'no_h0':
            r = {k: v for k, v in r.items() if not k.startswith('dh0_')}
        if variant == 'constant_gi':
            r = {k: (v.sum(0) if k.startswith('dx') else v) for k, v in r.items()}
        out.append(r)
    return tuple(out)

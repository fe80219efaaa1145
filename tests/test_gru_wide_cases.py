"""The case table of the streamed-weights GRU recurrences (gru_wide_cases.py) covers what it says, and the yardstick of its bars --
torch's fp32 CPU nn.GRU -- is within REL_CPU_MAX of float64 on every tensor of every case (except the host-BLAS sums, for which the
clamp in gru_cases.bar alone keeps the bar down).  No GPU.

Measured on one host at (256 | 512) x (6 | 24 steps) x (37 | 69 rows): the largest figure is 7.1e-7 (dweight_ih), outputs 2.6e-7 to
3.2e-7.  Every figure is printed."""
import pytest

import gru_cases as gc
import gru_wide_cases as wc


def test_table_covers_the_tiles_steps_counts_and_variants():
    hids = {c[0] for c in wc.CASES}
    assert hids == set(wc.HIDDEN) == {256, 512}
    rows = {c[2] for c in wc.CASES}
    assert rows <= set(wc.ROWS) and 5 in rows and 5 < min(wc.ROW_TILES)
    for rt in wc.ROW_TILES:                                    # a ragged last tile behind at least one full tile, at both hidden sizes
        for hid in wc.HIDDEN:
            assert any(c[0] == hid and c[2] % rt == 5 and c[2] > rt for c in wc.CASES), (rt, hid)
    assert {c[1] for c in wc.CASES} == set(wc.STEPS) == {1, 6, 24}
    for hid in wc.HIDDEN:
        assert {c[1] for c in wc.CASES if c[0] == hid} == {1, 6, 24}, hid
    assert {c[3] for c in wc.CASES} == {1, 2, 3, 4}
    assert {c[4] for c in wc.CASES} == set(wc.VARIANT_NAMES)
    assert gc.REVERSE == (False, True, False, True) and gc.NSEQ == 4
    assert [c for c in wc.CASES if c[4] == 'merged_gi'] and all(c[3] == 2 for c in wc.CASES if c[4] == 'merged_gi')
    assert len({wc.case_id(c) for c in wc.CASES}) == len(wc.CASES)


def test_chunks_cover_the_four_directions_once():
    for nseq in (1, 2, 3, 4):
        ch = wc.chunks(nseq)
        assert [i for a, b in ch for i in range(a, b)] == [0, 1, 2, 3] and all(1 <= b - a <= nseq for a, b in ch)


@pytest.mark.parametrize('case', wc.CASES, ids=wc.case_id)
def test_fp32_cpu_yardstick_is_within_1e6_of_float64(case):
    hid, steps, rows, _nseq, variant = case
    ref, cpu = wc.references(hid, steps, rows, variant)
    assert set(ref) == set(cpu) and ref
    assert ('dh0_0' in ref) == (variant != 'no_h0')
    slack = {}
    for k in ref:
        e = gc.rel(cpu[k], ref[k])
        print(f'{wc.case_id(case)} {k}: rel_cpu {e:.3e}')
        if gc.yardstick_is_held(k) and not e <= gc.REL_CPU_MAX:
            slack[k] = e
        assert gc.bar(k, e) <= (3e-6 if k.startswith(('y', 'hn')) else 2e-5)
    assert not slack, (wc.case_id(case), slack)

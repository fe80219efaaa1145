"""The case table of the GRU recurrences' float64 tests (gru_cases.py) checked on its own, without a GPU and without product code:
the row counts select the widths they are named for, they are ragged, and torch's fp32 CPU layer -- the yardstick of the bars -- is
within 1e-6 of float64 on every tensor of every case whose yardstick does not hang on the host's BLAS (gru_cases.py:
HOST_BLAS_SUMS), and the bars stay where that condition would put them: at most 3e-6 for outputs, the 2e-5 floor for gradients."""
import pytest

from gru_cases import (CASES, CUS, GRAD_FLOOR, NSEQ, OUT_R, REL_CPU_MAX, bar, chunk_rows, references, rel, rows_for, rows_per_wg,
                       yardstick_is_held)


@pytest.mark.parametrize('nseq', [1, 2, 3, 4])
def test_row_counts_select_their_width_and_are_ragged(nseq):
    for rw in (4, 8, 16):
        rows = rows_for(rw, nseq, CUS)
        assert rows_per_wg(rows, nseq, CUS) == rw, (rw, nseq, rows)
        assert rows % rw != 0 and rows > rw, (rw, nseq, rows)          # a ragged last workgroup behind at least one full one
    assert rows_per_wg(chunk_rows(nseq, CUS), nseq, CUS) == 4          # the chunks of the bitwise comparison run four rows wide
    assert rows_per_wg(chunk_rows(nseq, CUS) + 1, nseq, CUS) == 8      # ... and are the most that does


def test_restatement_at_the_thresholds():
    """gru_rows_per_wg at 256 CUs: one sequence changes width behind 1024 and 2048 rows (the tick decoder's launch), four behind
    256 and 512; the table's counts at four sequences are 21, 261 and 517 with 5 live rows in the last workgroup of 8 or 16"""
    assert [rows_per_wg(r, 1, 256) for r in (1, 1024, 1025, 2048, 2049, 100000)] == [4, 4, 8, 8, 16, 16]
    assert [rows_per_wg(r, 4, 256) for r in (256, 257, 512, 513)] == [4, 8, 8, 16]
    assert [rows_per_wg(r, 2, 256) for r in (512, 513, 1024, 1025)] == [4, 8, 8, 16]
    assert [rows_for(rw, 4, 256) for rw in (4, 8, 16)] == [21, 261, 517]
    assert 261 % 8 == 5 and 517 % 16 == 5


@pytest.mark.parametrize('hid,rw,steps', CASES, ids=[f'H{h}-RW{w}-T{t}' for h, w, t in CASES])
def test_fp32_cpu_layer_is_within_1e_6_of_float64(hid, rw, steps):
    ref, cpu = references(hid, steps, rows_for(rw, NSEQ, CUS))
    assert set(ref) == set(cpu) and len(ref) == 2 * (4 + 8)            # y, hn, dx, dh0 and eight parameter gradients per layer
    worst = {k: rel(cpu[k], ref[k]) for k in ref}
    print({k: f'{v:.2e}' for k, v in worst.items()})
    assert sum(not yardstick_is_held(k) for k in ref) == 4             # the four input projections' weight gradients, nothing else
    assert all(v <= REL_CPU_MAX for k, v in worst.items() if yardstick_is_held(k)), {k: v for k, v in worst.items() if v > REL_CPU_MAX}
    for k, v in worst.items():
        assert bar(k, v) <= (OUT_R * REL_CPU_MAX if k.startswith(('y', 'hn')) else GRAD_FLOOR), (k, v, bar(k, v))


def test_the_yardstick_cannot_inflate_a_bar():
    assert bar('y0', 1.0) == OUT_R * REL_CPU_MAX and bar('hn1', 0.0) == 2e-6 and bar('dx0', 1.0) == bar('dweight_ih_l0[0]', 3e-6) == GRAD_FLOOR
    assert bar('y0', 1e-3, clamp=False) == 3e-3 and bar('dh0_1', 1e-3, clamp=False) == 5e-3

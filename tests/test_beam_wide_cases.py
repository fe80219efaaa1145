"""The case table of the streamed-weights beam search's tests (beam_wide_cases.py) without a GPU: what it reaches, that its fp32 CPU
reference is a usable yardstick, and that every plan forces a tick."""
import numpy as np
import pytest

import gru_cases as gc
import beam_wide_cases as bc


def test_the_table_reaches_every_form_and_boundary():
    assert {c[5] for c in bc.CASES} == set(bc.FORMS)
    assert {c[0] for c in bc.CASES} == {256, 512}
    for hid in (256, 512):
        assert any(c[0] == hid and c[5] in ('planned', 'groups') for c in bc.CASES)
    rows = [c[1] * c[3] for c in bc.CASES]
    assert min(rows) < 32 and any(32 < r < 64 and r % 16 == 0 for r in rows) and any(r % 16 and r > 32 for r in rows)
    assert {1, 16} <= {c[3] for c in bc.CASES} and {2, 128} <= {c[2] for c in bc.CASES}
    assert any(c[2] % 16 == 1 for c in bc.CASES)                # a tile boundary in the vocabulary
    for c in bc.CASES:
        assert c[3] % c[4] == 0 and (c[4] > 1) == (c[5] == 'groups'), c       # G divides W
    shapes = [bc.shape(c) for c in bc.CASES]
    assert (2, 3) in shapes and any(tpb == 1 for _, tpb in shapes) and shapes.count((4, 6)) == len(shapes) - 2
    assert len({bc.case_id(c) for c in bc.CASES}) == len(bc.CASES)


@pytest.mark.parametrize('case', bc.CASES, ids=bc.case_id)
def test_fp32_reference_is_a_yardstick(case):
    p = bc.problem(*case)
    ref = bc.reference_logits(p, p['parents'], p['tokens'], np.float64)
    cpu = bc.reference_logits(p, p['parents'], p['tokens'], np.float32)
    assert ref.dtype == np.float64 and cpu.dtype == np.float32 and ref.shape == (p['batch'], p['ticks'], p['width'], p['vocab'])
    e = gc.rel(cpu, ref)
    print(f'{bc.case_id(case)}: rel_cpu {e:.3e}, largest logit {ref.max():.3f}, share of zero logits {(ref == 0).mean():.3f}')
    assert e <= gc.REL_CPU_MAX
    assert 0 < ref.max() and (ref == 0).mean() < 0.5            # ReLU outputs: mostly above zero


def test_the_reference_follows_the_parents():
    """beam k of a code whose parent and note are beam 0's repeats beam 0's logits at the next tick, and a restart forgets the parents"""
    case = bc.CASES[0]
    p = bc.problem(*case)
    parents, tokens = p['parents'].copy(), p['tokens'].copy()
    parents[:, 2, 1], tokens[:, 2, 1] = parents[:, 2, 0], tokens[:, 2, 0]
    ref = bc.reference_logits(p, parents, tokens, np.float64)
    np.testing.assert_array_equal(ref[:, 3, 1], ref[:, 3, 0])
    assert not np.array_equal(ref[:, 3, 2], ref[:, 3, 0])
    other = parents.copy()
    other[:, p['tpb'] - 1] = (other[:, p['tpb'] - 1] + 1) % p['width']
    np.testing.assert_array_equal(bc.reference_logits(p, other, tokens, np.float64)[:, p['tpb']], ref[:, p['tpb']])


def test_problems_hold_what_their_form_needs():
    for case in bc.CASES:
        p = bc.problem(*case)
        form, width = case[5], case[3]
        assert (p['allow'] is not None) == (form == 'masked') and (p['plan'] is not None) == (form in ('planned', 'groups'))
        if form == 'masked':
            assert width <= p['allow'].sum() < p['vocab']
        if p['plan'] is not None:
            n = p['plan'].astype(np.int64).sum(-1)
            assert (n[:, ::4] == 1).all() and (n >= 1).all()    # a forced tick every fourth, none empty
            rest = np.delete(n, np.arange(0, p['ticks'], 4), axis=1)
            assert rest.size == 0 or (rest >= 2).all()
        assert p['parents'].max() < width and p['tokens'].max() < p['vocab']

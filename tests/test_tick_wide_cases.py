"""The case table of the streamed-weights free-running tick decoder's tests (tick_wide_cases.py) without a GPU: what it reaches, that
its fp32 CPU reference is a usable yardstick, and that every note plan has the three kinds of tick."""
import numpy as np
import pytest

import gru_cases as gc
import tick_wide_cases as tc


def test_the_table_reaches_every_form():
    got = {(hid, form, masked) for hid, _, _, _, _, form, masked in tc.CASES}
    want = {(hid, form, False) for hid in tc.HIDDEN for form in tc.FORMS} | {(hid, form, True) for hid in tc.HIDDEN
                                                                              for form in ('argmax', 'multinomial')}
    assert got == want
    assert not any(masked and form not in ('argmax', 'multinomial') for _, _, _, _, _, form, masked in tc.CASES)
    assert {c[2] for c in tc.CASES} == set(tc.VOCABS) == {35, 70}
    assert {c[1] for c in tc.CASES} == set(tc.ROWS)
    assert all(r == 5 or (r % tile == 5 and r > tile) for r in tc.ROWS for tile in tc.ROW_TILES)
    assert {(c[3], c[4]) for c in tc.CASES} == {(4, 6), (1, 1)}
    assert sum((c[3], c[4]) == (1, 1) for c in tc.CASES) == 1
    for hid in tc.HIDDEN:                                       # both vocabularies and both row counts at either hidden size
        assert {c[2] for c in tc.CASES if c[0] == hid} == {35, 70} and {c[1] for c in tc.CASES if c[0] == hid} == {5, 37}
    assert len({tc.case_id(c) for c in tc.CASES}) == len(tc.CASES)


@pytest.mark.parametrize('case', tc.CASES, ids=tc.case_id)
def test_fp32_reference_is_a_yardstick(case):
    p = tc.problem(*case)
    ref = tc.reference_logits(p, p['tokens'], np.float64)
    cpu = tc.reference_logits(p, p['tokens'], np.float32)
    assert ref.dtype == np.float64 and cpu.dtype == np.float32 and ref.shape == (p['batch'], p['ticks'], p['vocab'])
    e = gc.rel(cpu, ref)
    print(f'{tc.case_id(case)}: rel_cpu {e:.3e}, largest logit {ref.max():.3f}, share of zero logits {(ref == 0).mean():.3f}')
    assert e <= gc.REL_CPU_MAX
    assert 0 < ref.max() and (ref == 0).mean() < 0.5            # ReLU outputs: mostly above zero


def test_problems_hold_what_their_form_needs():
    for case in tc.CASES:
        p = tc.problem(*case)
        form, masked = case[5], case[6]
        assert (p['mask'] is not None) == masked
        assert (p['uniforms'] is None) == (form == 'argmax')
        if p['uniforms'] is not None:
            assert p['uniforms'].min() > 0 and p['uniforms'].max() <= 1
        assert (p['allow'] is not None) == (form == 'filtered') and (p['plan'] is not None) == form.startswith('planned')
        if form == 'filtered':
            assert 0 < p['allow'].sum() < p['vocab'] and p['top_k'] < p['allow'].sum()
        if form == 'planned_argmax':
            assert p['top_k'] == 1 and bool((p['uniforms'] == 1).all())
        if masked:
            assert p['mask'].shape == (p['ticks'], p['batch'], p['hid']) and 0.4 < p['mask'].mean() < 0.6


def test_every_plan_has_the_three_kinds_of_tick():
    plans = [tc.problem(*c)['plan'] for c in tc.CASES if c[5].startswith('planned')]
    assert len(plans) == 4
    for plan in plans:
        forced, several, none = tc.plan_kinds(plan)
        assert forced > 0 and several > 0 and none == 1
        rows_with_none = np.nonzero((plan.sum(-1) == 0).any(-1))[0]
        assert len(rows_with_none) == 1                         # in one row, one tick

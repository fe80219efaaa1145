"""CPU proof for the float64 tests of the MeasureVAE lookup, segment-sum, tick-input and attribute kernels (sequence_cases.py,
test_sequence_kernels_float64.py):

  a. the float64 references reproduce torch float64 autograd of table[idx], of the gather G[prev] + G[beat row] + bias and of the
     reference tick formulation (W_ih0 [emb(prev) | beat_emb] + b_ih0 per tick, x_0 at tick 0), and the committed attribute golden;
  b. for every family and every case the fp32 yardstick itself and the fp32 restatement of the kernel's documented summation order
     pass the bar;
  c. the bar discriminates: every planted defect of sequence_cases.WRONG_KERNELS fails it on the cases named there;
  d. the LDS bound of the segment sum is the same in the host code (arvae_embed_bwd at dim 256, arvae_tick_gi_bwd) and in the three
     Python guards (Encoder._lookup_fits, HierarchicalDecoder._tick_lookup_fits, FusedMeasureVAE.fits).

Runs anywhere (no GPU)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sequence_cases as sc

torch.set_num_threads(1)


def close(a, b, rtol, atol=0.0):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


# ---------------------------------------------------------------------------------------------------------------- a. references
@pytest.mark.parametrize('case', sc.EMBED_CASES, ids=sc.case_id)
def test_embed_reference_is_torch_float64_autograd(case):
    inp = sc.embed_inputs(case)
    ref = sc.embed_ref(inp)
    batch, steps, vocab = inp['batch'], inp['steps'], inp['vocab']
    table = torch.from_numpy(inp['table']).double().requires_grad_(True)
    if inp['acc']:
        table.grad = torch.from_numpy(inp['old']).double().clone()
    out = table[torch.from_numpy(inp['idx']).clamp(0, vocab - 1)]               # (batch, steps, dim)
    if inp['tm']:
        out = out.transpose(0, 1)
    g = torch.from_numpy(inp['g']).double().view(out.shape)
    out.backward(g)
    assert np.array_equal(ref['x_out'], out.detach().numpy().reshape(batch * steps, -1).astype(np.float32))
    close(ref['dtable'], table.grad.numpy(), rtol=1e-12, atol=1e-13)
    # the table's planted tokens are there, and clamp where the header says
    if case[5] == 'out_of_range' and batch * steps >= 5:
        flat = inp['idx'].ravel()
        assert {-1, -7, vocab, vocab + 5, 2 ** 32 + 3} <= set(flat.tolist())
        rows = sc.embed_rows(inp)
        assert np.array_equal(ref['x_out'][rows[flat == 2 ** 32 + 3]], inp['table'][[vocab - 1]])
        assert np.array_equal(ref['x_out'][rows[flat == -7]], inp['table'][[0]])
    if case[5] in ('one_token', 'missing'):
        assert ref['x_unused_rows'].shape[0] >= vocab // 2 - 1


def test_embed_table_holds_every_value_the_kernels_branch_on():
    cases = sc.EMBED_CASES
    assert {c[0] for c in cases} >= {1, 10, 64, 100, 128, 129, 130, 132, 192, 768}
    assert {c[1] for c in cases} >= {1, 35, 63, 300} and all(c[0] <= sc.NARROW_MAX for c in cases if c[1] == 300)
    assert {c[2] for c in cases} >= {(1, 1), (1, 5), (1, 16), (1, 17), (2, 32), (3, 24), (37, 24), (86, 24)}
    assert {c[5] for c in cases} == {'uniform', 'one_token', 'missing', 'out_of_range'}
    for wide in (False, True):                                                    # each gradient kernel: both row orders, both modes
        mine = [c for c in cases if (c[0] > sc.NARROW_MAX) == wide]
        assert {(c[3], c[4]) for c in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert any(c[5] == 'out_of_range' for c in mine)
    assert any(c[0] % 4 and c[2][0] * c[2][1] * c[0] > sc.GRID_CAP for c in cases)
    assert len(set(cases)) == len(cases)


@pytest.mark.parametrize('case', [c for c in sc.TICK_GI_CASES if c[0][0] <= 86], ids=sc.case_id)      # (a graph node per row: not at 11000)
def test_tick_gi_reference_is_torch_float64_autograd(case):
    inp = sc.tick_gi_inputs(case)
    ref = sc.tick_gi_ref(inp)
    batch, beats, tpb, vocab = inp['batch'], inp['beats'], inp['tpb'], inp['vocab']
    g = torch.from_numpy(inp['g_small']).double().requires_grad_(True)
    tok = torch.from_numpy(inp['tokens']).clamp(0, vocab - 1)
    rows = []
    for j in range(tpb):                                                          # written out per row, not through tick_order()
        for beat in range(beats):
            for b in range(batch):
                t = tpb * beat + j
                rows.append(g[vocab if t == 0 else int(tok[b, t - 1])] + g[vocab + 1 + beat * batch + b])
    gi = torch.stack(rows)
    if inp['bias'] is not None:
        gi = gi + torch.from_numpy(inp['bias']).double()
    gi.backward(torch.from_numpy(inp['dgi']).double())
    close(ref['x_gi'], gi.detach().numpy(), rtol=3e-7, atol=1e-6)                 # (fp32 against float64)
    dg = g.grad.numpy()
    close(ref['dg_notes'], dg[:vocab], rtol=1e-12, atol=1e-13)
    close(ref['dg_x0'], dg[vocab], rtol=1e-12, atol=1e-13)
    close(ref['x_dg_beat'], dg[vocab + 1:], rtol=1e-5, atol=1e-5)
    # the x_0 row receives exactly the tick-0 gradients: rows (j = 0, beat = 0, b)
    close(ref['dg_x0'], inp['dgi'][:batch].astype(np.float64).sum(0), rtol=1e-12, atol=1e-13)


def test_tick_gi_table_holds_every_value():
    cases = sc.TICK_GI_CASES
    assert {c[0] for c in cases} >= {(1, 1, 1), (1, 4, 6), (3, 4, 6), (37, 4, 6), (5, 2, 12), (5, 1, 24), (7, 3, 8), (86, 4, 6)}
    assert {c[1] for c in cases} >= {4, 96, 192, 384, 260} and {c[2] for c in cases} >= {35, 1, 62}
    assert {c[3] for c in cases} == {'uniform', 'one_token', 'missing', 'out_of_range'} and {c[4] for c in cases} == {False, True}


@pytest.mark.parametrize('case', sc.TICK_PROJECTION_CASES, ids=sc.case_id)
def test_tick_projection_reference_is_torch_float64_autograd(case):
    inp = sc.tick_projection_inputs(case)
    ref, want = sc.tick_projection_ref(inp), sc.tick_projection_torch(inp, torch.float64)
    assert set(ref) == set(want)
    for k in ref:
        close(ref[k], want[k], rtol=1e-12, atol=1e-12)


def test_tick_rows_reference_is_the_block_matrix():
    for case in sc.TICK_ROWS_CASES:
        inp = sc.tick_rows_inputs(case)
        ref = sc.tick_rows_ref(inp)
        vocab, emb, hidden, rows, off = (inp[k] for k in ('vocab', 'emb', 'hidden', 'rows', 'off'))
        beat = inp['beat'][:, off:off + hidden]
        assert not (beat == sc.SENTINEL).any()
        want = np.block([[inp['table'], np.zeros((vocab, hidden), np.float32)], [inp['x0'][None], np.zeros((1, hidden), np.float32)],
                         [np.zeros((rows, emb), np.float32), beat]])
        assert np.array_equal(ref['x_x'], want)
        gaps = np.ones(inp['ld'], bool)
        gaps[off:off + hidden] = False
        assert (ref['x_dbeat'][:, gaps] == sc.SENTINEL).all() and np.array_equal(ref['x_dbeat'][:, ~gaps], inp['dx'][vocab + 1:, emb:])
        assert np.array_equal(ref['x_dtable'], inp['old_table'] if inp['null'] == 'dtable' else inp['old_table'] + inp['dx'][:vocab, :emb])
        assert np.array_equal(ref['x_dx0'], inp['old_x0'] if inp['null'] == 'dx0' else inp['old_x0'] + inp['dx'][vocab, :emb])
    big = [c for c in sc.TICK_ROWS_CASES if (c[0] + 1 + c[3]) * (c[1] + c[2]) > sc.GRID_CAP and (c[0] + 1) * c[1] + c[3] * c[2] > sc.GRID_CAP]
    assert big and {c[4] for c in sc.TICK_ROWS_CASES} == {'dense', 'hidden', 'executor'}


def test_copy_references_are_torchs_fp32_results():
    for case in sc.COPY_CASES:
        inp = sc.copy_inputs(case)
        ref = sc.copy_ref(inp)
        t = lambda a: torch.from_numpy(a)
        if inp['kind'] == 'concat':
            want = dict(x_out=torch.cat([t(inp['a']), t(inp['b'])], 1))
        elif inp['kind'] == 'split':
            gb = t(inp['g'])[:, inp['ca']:]
            want = dict(x_da=t(inp['g'])[:, :inp['ca']], x_db=t(inp['b']) + gb if inp['acc'] else gb)
        elif inp['kind'] == 'scale':
            v = torch.tensor(inp['alpha']) * t(inp['x'])
            v = v if inp['mask'] is None else v * t(inp['mask']).float()
            want = dict(x_y=t(inp['y']) + v if inp['acc'] else v)
        else:
            want = dict(x_y=t(inp['v'])[None].expand(inp['rows'], -1))
        assert set(ref) == set(want)
        for k in ref:
            assert ref[k].dtype == np.float32 and np.array_equal(ref[k], want[k].numpy()), (case, k)
    kinds = {c[0]: [x for x in sc.COPY_CASES if x[0] == c[0]] for c in sc.COPY_CASES}
    assert any(c[1] * sum(c[2]) > sc.GRID_CAP for c in kinds['concat']) and any(c[1] * sum(c[2]) > sc.GRID_CAP for c in kinds['split'])
    assert any(c[1] > sc.GRID_CAP for c in kinds['scale']) and any(c[1] * c[2] > sc.GRID_CAP for c in kinds['bcast'])
    assert {(c[2], c[3]) for c in kinds['scale']} == {(0, False), (0, True), (1, False), (1, True)}


def test_gru_gates_reference_is_torchs_gru_cell_in_float64():
    """the gate formulas against nn.GRUCell with identity projections: gi = W_ih x + b_ih, gh = W_hh h + b_hh supplied directly"""
    for case in sc.GRU_GATES_CASES:
        if case[1] > 100 or not case[2]:
            continue
        inp = sc.gru_gates_inputs(case)
        ref = sc.gru_gates_ref(inp)
        hid, batch = inp['hidden'], inp['batch']
        cell = torch.nn.GRUCell(3 * hid, hid).double()
        with torch.no_grad():                                                     # x = gi through an identity W_ih; gh = b_hh + 0 h is not
            cell.weight_ih.copy_(torch.eye(3 * hid))                              # expressible per row, so gh rides in through W_hh = 0 and
            cell.bias_ih.zero_()                                                  # one cell call per row with its own b_hh
            cell.weight_hh.zero_()
        for r in range(min(batch, 3)):
            with torch.no_grad():
                cell.bias_hh.copy_(torch.from_numpy(inp['gh'][r]).double())
            h = cell(torch.from_numpy(inp['gi'][r:r + 1]).double(), torch.from_numpy(inp['h_prev'][r:r + 1]).double())
            close(ref['h'][r], h.detach().numpy()[0], rtol=1e-12, atol=1e-14)
    assert any(c[3] >= 30 for c in sc.GRU_GATES_CASES) and any(c[0] * c[1] > sc.GRID_CAP for c in sc.GRU_GATES_CASES)


def test_attribute_reference_against_the_golden_and_table_coverage(golden_dir):
    g = np.load(os.path.join(golden_dir, 'attributes.npz'))
    score = g['score']
    tables = sc.attr_tables()
    w = sc.attr_inputs((24, 1))['w']
    inp = dict(steps=score.shape[1], batch=score.shape[0], vocab=len(tables[0]), score=score, tables=tables, w=w, norm=float(w.sum(dtype=np.float32)))
    ref = sc.attr_ref(inp)
    got = np.stack([ref['rhythm'], ref['x_range'], ref['x_density'], ref['x_contour']], 1)
    close(got, g['attr'], rtol=1e-6, atol=1e-7)
    seen = sc.attr_coverage()
    assert all(n >= 5 for n in seen.values()), seen
    assert {c[0] for c in sc.ATTR_CASES} == {1, 7, 8, 9, 24, 25} and {c[1] for c in sc.ATTR_CASES} == {1, 63, 64, 65, 130}
    # a one-note measure has range and contour 0
    inp = sc.attr_inputs((24, 65))
    ref = sc.attr_ref(inp)
    one = [r for r in range(65) if sc.attr_kind((24, 65), r) == 'one_note']
    assert one and not ref['x_range'][one].any() and not ref['x_contour'][one].any() and (ref['rhythm'][one] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- b. the bar passes
@pytest.mark.parametrize('family', list(sc.FAMILIES))
def test_yardstick_and_fp32_restatement_pass_the_bar_on_every_case(family):
    cases, inputs, ref_fn, cpu_fn, chain_fn = sc.FAMILIES[family]
    bad = []
    for case in cases:
        inp = inputs(case)
        ref, cpu = ref_fn(inp), cpu_fn(inp)
        assert set(cpu) >= set(ref), case
        bad += [(sc.case_id(case), 'yardstick', b) for b in sc.hold(sc.case_id(case) + ' [yardstick]', cpu, cpu, ref)]
        bad += [(sc.case_id(case), 'restatement', b) for b in sc.hold(sc.case_id(case) + ' [restatement]', chain_fn(inp), cpu, ref)]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- c. the bar discriminates
@pytest.mark.parametrize('name,family,case', [(n, f, c) for n, where in sc.WRONG_KERNELS.items() for f, c in where],
                         ids=lambda v: v if isinstance(v, str) else sc.case_id(v))
def test_the_bar_fails_a_wrong_kernel(name, family, case):
    cases, inputs, ref_fn, cpu_fn, chain_fn = sc.FAMILIES[family]
    assert case in cases, (name, case)
    inp = inputs(case)
    ref, cpu = ref_fn(inp), cpu_fn(inp)
    assert not sc.hold(sc.case_id(case) + ' [right]', chain_fn(inp), cpu, ref)
    bad = sc.hold(sc.case_id(case) + f' [{name}]', chain_fn(inp, name), cpu, ref)
    assert bad, (name, sc.case_id(case))


def test_wrong_kernel_list_covers_every_family_and_the_defects_the_tests_were_written_for():
    assert {f for where in sc.WRONG_KERNELS.values() for f, _ in where} == set(sc.FAMILIES)
    assert set(sc.WRONG_KERNELS) >= {'gradient index not clamped', 'batch-major rows read as time-major', 'last partial block dropped',
                                     'last position group dropped', 'accumulate overwrites', 'tick 0 takes token 0 instead of x_0',
                                     'beat rows summed over tpb - 1 ticks', 'beat row index b * beats + beat',
                                     'strided dbeat written densely', 'contour taken as first - last', 'one-note measure reports a range'}


# ---------------------------------------------------------------------------------------------------------------- d. the LDS bound
@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def _bound_sweep():
    """(entries, positions) either side of entries * 1024 + ceil(positions / 16) * 8 = 65536, and far from it"""
    out = []
    for entries in (1, 35, 36, 62, 63, 64, 65, 130):
        room = 65536 - entries * 1024
        edge = room // 8 * 16 if room > 0 else 0                                  # the largest position count that fits
        for positions in {1, 24, 2064, max(edge - 16, 1), max(edge - 1, 1), max(edge, 1), edge + 1, edge + 16, edge + 17, 100000}:
            out.append((entries, positions))
    return sorted(out)


def test_segment_sum_bound_is_the_same_in_host_code_and_python(lib):
    """pure host code: every library call below is refused before any launch and its pointers are never dereferenced (sizes the
    guards accept are not sent to the library: that would launch)"""
    from arvae_amd import ops
    from arvae_amd.fused_measure import FusedMeasureVAE
    from arvae_amd.measure_vae import Encoder, HierarchicalDecoder
    fake = ctypes.c_void_p(256)
    fits_seen = refused_seen = 0
    for entries, positions in _bound_sweep():
        want = entries * 1024 + (positions + 15) // 16 * 8 <= 65536               # sequence.hip: nv * 256 floats + 2 ints per position of a group
        assert ops.segment_sum_fits(entries, positions) == want
        # the encoder's lookup: entries = vocabulary, positions = steps * batch
        assert Encoder._lookup_fits(SimpleNamespace(num_notes=entries), 1, positions) == want
        if positions % 24 == 0:
            assert Encoder._lookup_fits(SimpleNamespace(num_notes=entries), 24, positions // 24) == want
        # the decoder's and the executor's: entries = vocabulary + 1 (x_0)
        dec = SimpleNamespace(num_notes=entries - 1, rnn_hidden_size=128)
        assert HierarchicalDecoder._tick_lookup_fits(dec, positions) == want
        if positions % 24 == 0:
            fused = SimpleNamespace(model=SimpleNamespace(num_notes=entries - 1, num_ticks_per_measure=24))
            assert FusedMeasureVAE.fits(fused, positions // 24) == want
        if want:
            fits_seen += 1
            continue
        refused_seen += 1
        assert lib.arvae_embed_bwd(fake, fake, 1, positions, 256, entries, 1, fake, 0, fake, None) == -1
        assert b'do not fit' in lib.arvae_last_error_string(), (entries, positions)
        if entries >= 2:
            assert lib.arvae_tick_gi_bwd(fake, fake, 1, 1, positions, entries - 1, 384, fake, fake, None) == -1
            assert b'do not fit' in lib.arvae_last_error_string(), (entries, positions)
    assert fits_seen >= 10 and refused_seen >= 10
    # the model's sizes: 35 notes at batch 256 fit everywhere; 62 notes + x_0 fit up to 2048 ticks, one measure of 24 less than 86
    assert ops.segment_sum_fits(36, 24 * 256) and ops.segment_sum_fits(63, 24 * 85) and not ops.segment_sum_fits(63, 24 * 86)
    assert not HierarchicalDecoder._tick_lookup_fits(SimpleNamespace(num_notes=35, rnn_hidden_size=1), 24)     # 3 floats a row: no float4

"""tests/workspace_cases.py on the CPU: the table reaches scratch in every family (the size functions are host code), holds the
shapes its docstrings promise, and its exceptions name single buffers of existing cases."""
import importlib
import inspect
import re

import pytest

import single_channel_cases as sc
import split_cases as sp
import workspace_cases as wc


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def sizes(lib):
    return {c.name: [int(s) for s in c.sizes(lib)] for c in wc.CASES}


def test_every_family_has_a_case_that_uses_scratch(sizes):
    """a table that silently exercises no scratch fails here, not on the GPU"""
    assert {c.family for c in wc.CASES} == set(wc.FAMILIES)
    for family in wc.FAMILIES:
        with_scratch = [c.name for c in wc.CASES if c.family == family and max(sizes[c.name], default=0) > 0]
        print(f'{family}: {len(with_scratch)} of {sum(c.family == family for c in wc.CASES)} cases report scratch')
        assert with_scratch, family


def test_every_size_function_answers(sizes):
    for name, got in sizes.items():
        assert got and all(s >= 0 for s in got), (name, got)


def test_the_scratch_paths_the_table_is_there_for_report_scratch(sizes):
    """the weight gradients of every link family, the folded operands' AMAX pass, the split reductions, every decoder, both
    executors: each of these cases must reach a non-empty workspace"""
    must = [n for n in sizes if '-wgrad' in n or n.startswith(('conv32-', 'wgrad-', 'channel_sum-', 'wide_dense-', 'tick_', 'classify-', 'ksg_',
                                                                 'dsprites-', 'mnist-', 'measure-', 'reg-', 'image-', 'token-'))]
    must += [n for n in sizes if n.startswith('c64_25-n3-')]
    assert len(must) > 100
    for name in must:
        assert max(sizes[name]) > 0, (name, sizes[name])


def test_link_families_hold_the_shapes_they_promise():
    names = set(wc.BY_NAME)
    assert {f'conv32-lo{s}-n{n}' for s in (16, 8, 4) for n in (1, 5)} <= names
    assert {f'{link}-n3' for link in sp.CONV_LINKS} <= names
    for link in {name for name, _ in sp.WGRAD_CASES}:
        n_max = max(n for name, n in sp.WGRAD_CASES if name == link)
        assert {f'{link}-wgrad-n1', f'{link}-wgrad-n{n_max}'} <= names
    assert {'c64_31', 'c64_k3'} <= {name for name, _ in sp.WGRAD_CASES}
    folded = [n for n in names if n.startswith('c64_25-n3-')]
    assert len(folded) == 8                                     # act 1, 2 x keep-mask or not x either side
    picked = wc._single_channel_selection()
    assert {c.kernel for c in picked} == {c.kernel for c in sc.CASES}
    assert [c for c in sc.OUTSIDE_CASES if c not in picked] == []
    generic = [c for c in picked if c.geom == wc.GENERIC_WGRAD]
    assert sorted(c.n for c in generic) == [1, 2, 3]
    g = wc.GENERIC_WGRAD
    assert g.lw == 29 and g.lh * g.lw == 841 and (3 * 841) % 32 != 0 and (3 * 841) % 16 != 0


def test_row_counts_and_sizes_of_the_other_families():
    names = set(wc.BY_NAME)
    assert {f'channel_sum-r{r}-c{c}' for r in (1, 15, 17, 16385) for c in (8, 64, 10)} <= names and 'channel_sum-r17-c64-folded' in names
    assert (16385 + 15) // 16 > 1024                            # above the block clamp: rpb > 16
    assert sum(n.startswith('wide_dense-') for n in names) == 12 and {'wide_dense-5x2888to256-mode0', 'wide_dense-1100x256to2888-mode2'} <= names
    assert {'dense-2050x138to384', 'dense-2048x256to130', 'dense-33x256to10-deferred'} <= names
    assert 'gru_sequence-H32-T6-R21' in names
    for hid, vocab in wc.TICK_SIZES:
        for batch, beats, tpb in wc.TICK_SHAPES:
            tail = f'H{hid}-V{vocab}-B{batch}-{beats}x{tpb}'
            assert {f'tick_free_run-{f}-{tail}' for f in ('argmax', 'uniforms', 'filtered', 'planned')} <= names
            assert {f'tick_beam_search-{f}-{tail}' for f in ('plain', 'planned', 'groups')} <= names
    assert not [n for n in names if re.search(r'layers-.*-L[34]-H128', n)]      # kept on the tick-by-tick path
    assert [n for n in names if '-L3-H64-' in n] and [n for n in names if '-L1-H128-' in n]
    assert {'classify-n1', 'classify-n3', 'ksg_mi-n301-k3'} <= names
    assert {'dsprites-b3-train_step', 'dsprites-b37-train_step', 'dsprites-b37-eval_forward', 'mnist-b37-train_step', 'mnist-b37-eval_forward',
            'measure-b21-teacher_forced-train_step', 'measure-b21-free_running-train_step', 'measure-b21-free_running-eval_forward'} <= names
    assert all(c.family == wc.EXECUTOR_FAMILY for c in wc.CASES if c.name.startswith(('dsprites-', 'mnist-', 'measure-')))


def test_layer_predicates_agree_with_the_table(lib):
    """the table skips exactly what the library does not offer"""
    for hid, vocab in wc.TICK_SIZES:
        assert lib.arvae_tick_free_run_supported(hid, vocab)
        assert lib.arvae_tick_beam_search_groups_supported(hid, vocab, wc.BEAM_WIDTH, wc.BEAM_GROUPS)
        assert not lib.arvae_tick_free_run_layers_supported(hid, vocab, 2)          # two layers: arvae_tick_free_run
        for layers in (1, 3):
            offered = bool(lib.arvae_tick_free_run_layers_supported(hid, vocab, layers))
            assert offered == any(f'-L{layers}-H{hid}-' in n for n in wc.BY_NAME), (hid, layers)


def test_exceptions_name_one_buffer_of_one_case_each():
    seen = set()
    for row in wc.EXCEPTIONS:
        case, key, site, why = row
        assert case in wc.BY_NAME and '*' not in case + key + site and key and re.fullmatch(r'[\w.]+\.py:\d+ \(\w+\)', site), row
        module, line, function = re.fullmatch(r'([\w.]+)\.py:(\d+) \((\w+)\)', site).groups()
        source, first = inspect.getsourcelines(getattr(importlib.import_module('arvae_amd.' + module), function))
        assert first <= int(line) < first + len(source), f'{row}: line {line} is outside {function} ({module}.py:{first}-{first + len(source) - 1})'
        assert re.search(r'\w+\.(py|hip|h):\d+', why), f'{row}: the reason names the code line that makes it so'
        assert (case, key) not in seen
        seen.add((case, key))
    assert len(wc.EXCEPTIONS) <= 4

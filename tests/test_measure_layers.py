"""MeasureVAE at GRU layer counts other than two (--num_encoder_layers / --num_decoder_layers), the part that needs no GPU:
construction against the reference's recorded state_dict and repr, the C ABI of the layer-count tick decoder, and the float64
restatement tests/layer_stack_ref.py against the reference's goldens (tests/golden/make_layer_goldens.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from arvae_amd import synthetic as syn
from oracle import attributes as o_attr
from oracle import measure_vae as o_mvae

import layer_stack_ref as ref

LAYER_CASES = [(1, 1, 64, 20, 'tf'), (1, 1, 64, 20, 'free'), (3, 3, 64, 20, 'tf'), (3, 3, 64, 20, 'free'), (1, 3, 128, 21, 'free'),
               (3, 1, 128, 21, 'eval')]
CASE_IDS = [f'e{c[0]}d{c[1]}_{c[4]}' for c in LAYER_CASES]


class _FolkDataset:
    """the attributes MeasureVAE / MeasureVAETrainer read from the reference's FolkNBarDataset"""
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


def golden_state(enc_layers, dec_layers, hid):
    """the weights of a golden case: synthetic seed 4, logits spread as in measure_step_*.npz"""
    state = syn.synth_state(ref.shapes(enc_layers, dec_layers, hid), 4)
    state['decoder.tick_emb_to_note_emb.0.bias'] = state['decoder.tick_emb_to_note_emb.0.bias'] + np.float32(0.5)
    state['decoder.tick_emb_to_note_emb.0.weight'] = state['decoder.tick_emb_to_note_emb.0.weight'] * np.float32(3.0)
    return state


def golden_case(golden_dir, case):
    """-> (golden arrays, state, score, eps) of a LAYER_CASES entry"""
    enc_layers, dec_layers, hid, batch, mode = case
    g = np.load(os.path.join(golden_dir, f'measure_layers_e{enc_layers}d{dec_layers}_{mode}.npz'))
    score = syn.measure_batch(batch, seed=6 if mode == 'eval' else 5)
    eps = syn.normal_noise((batch, 32), seed=int(g['eseed']))
    return g, golden_state(enc_layers, dec_layers, hid), score, eps


@pytest.fixture(scope='module')
def struct(golden_dir):
    with open(os.path.join(golden_dir, 'measure_layers_struct.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('enc_layers,dec_layers', [(1, 1), (3, 3), (4, 4), (1, 3), (3, 1)])
def test_construction_matches_the_reference(struct, enc_layers, dec_layers):
    """keys, shapes, registration order and repr strings of the reference's model at these layer counts"""
    from arvae_amd.measure_vae import MeasureVAE
    want = struct[f'e{enc_layers}d{dec_layers}']
    model = MeasureVAE(_FolkDataset(), 10, 2, enc_layers, 64, 0.0, 32, dec_layers, 64, 0.0, False, 'folk')
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == want['keys']
    assert repr(model.encoder) == want['encoder_repr'] and repr(model.decoder) == want['decoder_repr']
    assert repr(model) == want['model_repr']
    assert got == [[k, list(s)] for k, s in ref.shapes(enc_layers, dec_layers, 64).items()]      # (the test helper's own table)
    assert len(model.arena_parameters()) == len(list(model.parameters()))


def test_two_layers_are_unchanged(struct):
    from arvae_amd.measure_vae import Encoder, HierarchicalDecoder, MeasureVAE
    model = MeasureVAE(_FolkDataset(), 10, 2, 2, 64, 0.0, 32, 2, 64, 0.0, False, 'folk')
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == struct['e2d2']['keys'] == [[k, list(s)] for k, s in o_mvae.shapes(hid=64).items()]
    assert repr(model.encoder) == struct['e2d2']['encoder_repr'] and repr(model.decoder) == struct['e2d2']['decoder_repr']
    with pytest.raises(NotImplementedError):
        Encoder(10, 64, 2, 35, 0.0, False, 32)                 # the reference's MeasureVAE never builds a unidirectional encoder
    with pytest.raises(ValueError):
        Encoder(10, 64, 0, 35, 0.0, True, 32)
    with pytest.raises(ValueError):
        HierarchicalDecoder(10, 35, 32, 0, 64, 0.0)


def test_dropout_mask_shapes():
    """one keep-mask per layer boundary; two layers also take today's shapes; one layer has no boundary and refuses a push"""
    from arvae_amd.measure_vae import Encoder, HierarchicalDecoder, _boundary_masks
    with pytest.raises(ValueError):
        Encoder(10, 32, 1, 35, 0.5, True, 32).push_dropout_mask(torch.ones(24, 5, 64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        HierarchicalDecoder(10, 35, 32, 1, 32, 0.5).push_dropout_masks(torch.ones(4, 5, 32, dtype=torch.uint8), torch.ones(24, 5, 32, dtype=torch.uint8))
    m = torch.ones(24, 5, 64, dtype=torch.uint8)
    assert len(_boundary_masks(m, 2, (24, 5, 64), 'tick')) == 1
    assert len(_boundary_masks(m[None], 2, (24, 5, 64), 'tick')) == 1
    assert [tuple(k.shape) for k in _boundary_masks(torch.ones(2, 24, 5, 64, dtype=torch.uint8), 3, (24, 5, 64), 'tick')] == [(24, 5, 64)] * 2
    with pytest.raises(ValueError):
        _boundary_masks(m, 3, (24, 5, 64), 'tick')


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_layers_supported_truth_table(lib):
    for hidden in (16, 32, 48, 64, 128, 256):
        for vocab in (0, 1, 16, 32, 33, 35, 64, 65):
            base = lib.arvae_tick_free_run_supported(hidden, vocab)
            assert base == int(hidden in (32, 64, 128) and 1 <= vocab <= min(64, 16 * (hidden // 16)))
            for layers in range(0, 7):
                assert lib.arvae_tick_free_run_layers_supported(hidden, vocab, layers) == int(bool(base) and layers in (1, 3, 4) and not (hidden == 128 and layers >= 3)), \
                    (hidden, vocab, layers)
    for layers, mats in ((1, 1), (3, 5), (4, 7)):
        for hidden in (32, 64, 128):                           # 2L - 1 matrices of 3H x H as two fp16 terms, their maxima behind
            n = lib.arvae_tick_free_run_layers_ws_floats(hidden, layers)
            assert n >= mats * 3 * hidden * hidden + mats and n % 4 == 0
    assert lib.arvae_tick_free_run_layers_ws_floats(48, 3) == 0 and lib.arvae_tick_free_run_layers_ws_floats(128, 5) == 0
    assert lib.arvae_tick_free_run_layers_ws_floats(128, 0) == 0


def test_tick_stack_struct_matches_the_header(tmp_path):
    """sizeof / field offsets of arvae_tick_stack_t as gcc lays it out == the ctypes mirror (as tests/test_abi.py does for the others)"""
    import shutil
    import subprocess
    from arvae_amd import _lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('gcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ['layers', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'w_out', 'b_out', 'h0', 'h0_stride']
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{root}/include/arvae_hip.h"', 'int main(void) {',
             r'printf("%zu %d\n", sizeof(arvae_tick_stack_t), ARVAE_TICK_MAX_LAYERS);']
    lines += [rf'printf("%zu\n", offsetof(arvae_tick_stack_t, {f}));' for f in fields] + ['return 0; }']
    src = tmp_path / 'sizes.c'
    src.write_text('\n'.join(lines))
    subprocess.run([gcc, '-o', str(tmp_path / 'sizes'), str(src)], check=True)
    out = subprocess.run([str(tmp_path / 'sizes')], check=True, capture_output=True, text=True).stdout.split()
    assert [int(out[0]), int(out[1])] == [ctypes.sizeof(_lib.TickStack), _lib.TICK_MAX_LAYERS]
    assert [int(v) for v in out[2:]] == [getattr(_lib.TickStack, f).offset for f in fields]


def test_tick_free_run_layers_rejects_bad_arguments(lib):
    from arvae_amd._lib import TickStack
    p = ctypes.c_void_p(256)                                   # never dereferenced: every call below fails validation first
    tok = (ctypes.c_int64 * 24)()

    def stack(layers, holes=()):
        s = TickStack()
        s.layers = layers
        for l in range(min(layers, 4)):
            s.w_ih[l], s.w_hh[l], s.b_ih[l], s.b_hh[l], s.h0[l] = 256, 256, 256, 256, 256
        s.w_out, s.b_out = 256, 256
        for name, l in holes:
            getattr(s, name)[l] = None
        return s

    def call(s, hidden=64, vocab=35, uniforms=None, inv_t=1.0, ws=p, gib=p, batch=1, mask=None, keep_scale=1.0, h0_stride=0):
        if s is not None:
            s.h0_stride = h0_stride
        return lib.arvae_tick_free_run_layers(None if s is None else ctypes.byref(s), gib, p, mask, keep_scale, batch, 4, 6, hidden, vocab,
                                              uniforms, inv_t, ctypes.cast(tok, ctypes.c_void_p), ws, None)

    def err():
        return lib.arvae_last_error_string()
    assert call(None) == -1 and b'null' in err()
    assert call(stack(3), gib=None) == -1 and b'null' in err()
    assert call(stack(3), ws=None) == -1 and b'workspace' in err()
    assert call(stack(3), ws=ctypes.c_void_p(260)) == -1 and b'aligned' in err()
    assert call(stack(0)) == -1 and call(stack(5)) == -1 and b'layers' in err()
    assert call(stack(2)) == -1 and b'arvae_tick_free_run' in err()           # two layers have their own entry point
    assert call(stack(3), hidden=128) == -1 and call(stack(4), hidden=128) == -1 and b'not offered' in err()   # 128 wide: three and four layers go tick by tick
    assert call(stack(3), hidden=64, h0_stride=32) == -1 and b'h0_stride' in err()
    assert call(stack(3), hidden=64, mask=p, keep_scale=float('nan')) == -1 and b'keep scale' in err()
    assert call(stack(3), hidden=48) == -1 and b'hidden size' in err()
    assert call(stack(3), vocab=65) == -1 and call(stack(1), hidden=32, vocab=35) == -1 and b'vocabulary' in err()
    assert call(stack(3), batch=0) == -1 and b'empty' in err()
    assert call(stack(3, holes=[('w_hh', 2)])) == -1 and b'layer 2' in err()
    assert call(stack(3, holes=[('h0', 1)])) == -1 and b'layer 1' in err()
    assert call(stack(3, holes=[('w_ih', 1)])) == -1 and b'layer 1' in err()
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        assert call(stack(3), uniforms=p, inv_t=bad) == -1 and b'temperature' in err()
    # layer 0's input weights are not read (gib / ptab hold their products): a hole there is not an error of validation -- the
    # call gets as far as the launch, which fails without a device or runs into these dummy pointers with one: not made here


def test_executor_reason_for_other_layer_counts():
    from arvae_amd.fused_measure import FusedMeasureVAE
    from arvae_amd.measure_vae import MeasureVAE
    for enc_layers, dec_layers in ((1, 2), (2, 3), (3, 1)):
        model = MeasureVAE(_FolkDataset(), 10, 2, enc_layers, 64, 0.0, 32, dec_layers, 64, 0.0, False, 'folk')
        assert FusedMeasureVAE.supports(model, None, (0, 1, 2, 3)) == 'layer count not built in the executor'


@pytest.mark.parametrize('case', LAYER_CASES, ids=CASE_IDS)
def test_restatement_vs_reference_goldens(golden_dir, case):
    """tests/layer_stack_ref.py (float64) against the reference's float32 CPU step.  Bars: the reference's own rounding -- a loss term
    is a mean over 24 B cross-entropies of fp32 logits behind <= 28 chained GRU steps, a few 1e-6 relative (2e-5 allowed); z, mu at
    1e-5 relative + 1e-5 absolute (fp32 heads behind the encoder's 24-step chains; |z| reaches 20 with these weights); a parameter's gradient norm sums fp32 products over the same chains (1e-3, half the 2e-3 the
    GPU path is allowed against the same goldens); the fed-back notes are exact (the generator asserts a top-1 margin > 1e-4)."""
    g, state, score, eps = golden_case(golden_dir, case)
    mode = case[4]
    assert float(g['margin']) > 1e-4
    attr = o_attr.attribute_labels(score, *syn.measure_tables())
    np.testing.assert_allclose(attr, g['attr'], rtol=1e-6)         # (fp32 sums in another order: an ulp)
    out = ref.step(state, score, eps, attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, mode == 'tf')
    for k in ('recons', 'dist', 'reg', 'loss', 'acc'):
        np.testing.assert_allclose(out[k], float(g[k]), rtol=2e-5, err_msg=k)
    np.testing.assert_array_equal(out['samples'], g['samples'])
    np.testing.assert_allclose(out['z'], g['z'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out['mu'], g['mu'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out['sigma'], g['sigma'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out['weights'][0], g['weights_row0'], rtol=1e-4, atol=1e-5)
    for name in state:
        gr = out['grads'][name].ravel()
        gn = float(g[f'gnorm/{name}'])
        np.testing.assert_allclose(np.sqrt((gr * gr).sum()), gn, rtol=1e-3, atol=1e-12, err_msg=name)
        samp = gr[syn.sample_indices(name, gr.size)]
        assert np.abs(samp - g[f'gsamp/{name}']).max() <= 1e-3 * max(np.abs(gr).max(), 1e-30) + 1e-9, name


def test_restatement_masks_act_between_layers_only():
    """explicit keep-masks reach every boundary and nothing else: all-ones masks at scale 1 change nothing, a zero mask on the LAST
    boundary cuts the top layer off from its input (its outputs then do not depend on the score through the lower layers)"""
    state = golden_state(3, 3, 32)
    p = {k: torch.from_numpy(v).double() for k, v in state.items()}
    score = torch.from_numpy(syn.measure_batch(3, seed=9))
    plain = ref.encode(p, score)
    ones = torch.ones(2, 24, 3, 64, dtype=torch.uint8)
    same = ref.encode(p, score, ones, keep_scale=1.0)
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    doubled = ref.encode(p, score, ones, keep_scale=2.0)
    assert not torch.equal(plain[0], doubled[0])
    z = torch.from_numpy(syn.normal_noise((3, 32), seed=2)).double()
    w_plain, _ = ref.decode(p, z, score, True)
    w_ones, _ = ref.decode(p, z, score, True, torch.ones(2, 4, 3, 32, dtype=torch.uint8), torch.ones(2, 24, 3, 32, dtype=torch.uint8), 1.0)
    assert torch.equal(w_plain, w_ones)
    cut = torch.ones(2, 24, 3, 32, dtype=torch.uint8)
    cut[1] = 0
    other = torch.from_numpy(syn.measure_batch(3, seed=10))
    w_a, _ = ref.decode(p, z, score, True, None, cut)
    w_b, _ = ref.decode(p, z, other, True, None, cut)
    assert torch.equal(w_a, w_b) and not torch.equal(w_plain, w_a)

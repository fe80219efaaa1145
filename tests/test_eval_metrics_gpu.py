"""The disentanglement metrics on the device (csrc/ksg.hip, arvae_amd.evaluation) against a NumPy brute force and against the
reference's metric suite as recorded in tests/golden/eval_metrics_*.npz (tests/golden/make_eval_goldens.py: the reference's
utils/evaluation.py with sklearn / scipy, the c-th KSG call pinned to RandomState(seed + c)); the trainers' and the CLIs'
evaluation paths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arvae_amd  # noqa: F401
from arvae_amd import evaluation as ev
from arvae_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_eval_metrics import brute_force_ksg  # noqa: E402

KINDS = ('small', 'dsprites', 'mnist', 'measure')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


_RUNS = {}


def suite(kind, golden_dir):
    """(golden, metrics with details) of one shape, computed once per module"""
    if kind not in _RUNS:
        g = np.load(os.path.join(golden_dir, f'eval_metrics_{kind}.npz'))
        codes, attrs, names = syn.eval_metric_inputs(kind, 0)
        _RUNS[kind] = (g, ev.compute_disentanglement_metrics(codes, attrs, names, random_state=int(g['seed']), return_details=True))
    return _RUNS[kind]


def test_radii_and_counts_equal_a_brute_force(dev):
    """radius_out bit-equal, nx_out / ny_out identical to the dense fp64 restatement: a three-level attribute, one with exact
    zeros, a continuous one, and each attribute against itself (the entropy case)"""
    codes, attrs, _ = syn.eval_metric_inputs('small', 0)
    for a in range(attrs.shape[1]):
        for X, seed in ((codes, 3 + a), (attrs[:, a:a + 1], 11 + a)):
            Xp, yp = ev.prepare_inputs(X, attrs[:, a], np.random.RandomState(seed))
            x_cols = torch.from_numpy(np.ascontiguousarray(Xp.T)).to(dev)
            mi, radius, nx, ny = ev.ksg_mi(x_cols, torch.from_numpy(yp.astype(np.float64)).to(dev), 3, with_details=True)
            mi, radius, nx, ny = mi.cpu().numpy(), radius.cpu().numpy(), nx.cpu().numpy(), ny.cpu().numpy()
            for c in range(Xp.shape[1]):
                want_mi, want_r, want_nx, want_ny = brute_force_ksg(Xp[:, c], yp, 3)
                assert np.array_equal(radius[c].view(np.uint64), want_r.view(np.uint64)), (a, c)
                assert np.array_equal(nx[c], want_nx) and np.array_equal(ny[c], want_ny), (a, c)
                assert abs(mi[c] - want_mi) <= 1e-12


def test_other_neighbour_counts_and_strided_columns(dev):
    """k = 1 and k = 8 (the extremes the entry accepts), columns at a stride ldx > n"""
    import ctypes
    from arvae_amd import _lib
    codes, attrs, _ = syn.eval_metric_inputs('small', 1)
    Xp, yp = ev.prepare_inputs(codes[:301], attrs[:301, 0], np.random.RandomState(2))
    n, p, ldx = 301, Xp.shape[1], 320
    padded = torch.full((p, ldx), float('nan'), dtype=torch.float64, device=dev)
    padded[:, :n] = torch.from_numpy(np.ascontiguousarray(Xp.T)).to(dev)
    y = torch.from_numpy(yp.astype(np.float64)).to(dev)
    lib = _lib.load()
    for k in (1, 8):
        ws = torch.empty(lib.arvae_ksg_ws_bytes(n, p), dtype=torch.uint8, device=dev)
        mi = torch.empty(p, dtype=torch.float64, device=dev)
        radius = torch.empty((p, n), dtype=torch.float64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.arvae_ksg_mi(ev._ptr(padded), ldx, p, ev._ptr(y), n, k, ev._ptr(ws), ev._ptr(mi), ev._ptr(radius), None, None,
                                    stream), 'ksg_mi')
        for c in range(p):
            want_mi, want_r, _, _ = brute_force_ksg(Xp[:, c], yp, k)
            assert np.array_equal(radius[c].cpu().numpy(), want_r) and abs(float(mi[c]) - want_mi) <= 1e-12, (k, c)


@pytest.mark.parametrize('kind', KINDS)
def test_every_ksg_call_matches_the_reference(dev, golden_dir, kind):
    g, m = suite(kind, golden_dir)
    d = m['_details']
    for key in ('mi_interp', 'mi_mod', 'mi_mig', 'entropy'):
        assert d[key].shape == g[key].shape
        np.testing.assert_allclose(d[key], g[key], rtol=0, atol=1e-10, err_msg=key)


@pytest.mark.parametrize('kind', KINDS)
def test_metrics_match_the_reference(dev, golden_dir, kind):
    g, m = suite(kind, golden_dir)
    d = m['_details']
    np.testing.assert_allclose(d['scc'], g['scc'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(d['sap'], g['sap'], rtol=0, atol=1e-9)
    interp_mean, corr, modularity, mig, sap = g['scalars']
    names = [f'attr{a}' for a in range(g['interp'].shape[0])]
    assert [m['interpretability'][n][0] for n in names] == [int(v) for v in g['interp'][:, 0]]
    for n, (_, score) in zip(names, g['interp']):
        assert abs(m['interpretability'][n][1] - score) <= 1e-5          # the reference fits its R^2 in float32
    assert abs(m['interpretability']['mean'][1] - interp_mean) <= 1e-5
    assert abs(m['Corr_score'] - corr) <= 1e-9
    assert abs(m['modularity_score'] - modularity) <= 1e-9
    assert abs(m['mig'] - mig) <= 1e-9
    assert abs(m['SAP_score'] - sap) <= 1e-9


@pytest.mark.parametrize('kind', ('small', 'dsprites'))
def test_same_random_state_is_bit_identical(dev, golden_dir, kind):
    _, first = suite(kind, golden_dir)
    codes, attrs, names = syn.eval_metric_inputs(kind, 0)
    again = ev.compute_disentanglement_metrics(codes, attrs, names, random_state=17, return_details=True)
    for key, v in first['_details'].items():
        assert np.array_equal(v.view(np.uint64), again['_details'][key].view(np.uint64)), key
    first = {k: v for k, v in first.items() if k != '_details'}
    again = {k: v for k, v in again.items() if k != '_details'}
    assert json.dumps(first) == json.dumps(again)


def test_standalone_functions_agree_with_the_suite(dev, golden_dir):
    """the reference's public names, one by one, on the calls they make themselves (an int seed counts from each function's
    first KSG call)"""
    g, m = suite('small', golden_dir)
    codes, attrs, names = syn.eval_metric_inputs('small', 0)
    a, s = attrs.shape[1], int(g['seed'])
    assert ev.compute_interpretability_metric(codes, attrs, names, random_state=s) == m['interpretability']
    assert ev.compute_correlation_score(codes, attrs) == {'Corr_score': m['Corr_score']}
    assert ev.compute_modularity(codes, attrs, random_state=s + a) == {'modularity_score': m['modularity_score']}
    assert ev.compute_mig(codes, attrs, random_state=s + 2 * a) == {'mig': m['mig']}
    assert ev.compute_sap_score(codes, attrs) == {'SAP_score': m['SAP_score']}
    np.testing.assert_array_equal(ev.continuous_mutual_info(codes, attrs, random_state=s + a), m['_details']['mi_mod'].T)
    assert np.array_equal(ev.continuous_entropy(attrs, random_state=s + 3 * a), m['_details']['entropy'])
    np.testing.assert_array_equal(ev.mutual_info_regression(codes, attrs[:, 1], random_state=s + 1), m['_details']['mi_interp'][1])


REFERENCE_KEYS = {'interpretability', 'Corr_score', 'modularity_score', 'mig', 'SAP_score'}


def _check_results(trainer, metrics, folder, seed):
    assert REFERENCE_KEYS | {'representations', 'test_loss', 'test_acc'} <= set(metrics)
    on_disk = json.load(open(os.path.join(folder, 'results_dict.json')))
    assert on_disk == metrics
    rec = json.load(open(os.path.join(folder, 'representations.json')))
    want = ev.json_ready(ev.compute_disentanglement_metrics(np.asarray(rec['latent_codes'], np.float32),
                                                            np.asarray(rec['attributes'], np.float32), rec['attr_list'],
                                                            random_state=seed))
    assert {k: metrics[k] for k in REFERENCE_KEYS} == want
    assert set(metrics['interpretability']) == set(rec['attr_list']) | {'mean'}
    return on_disk


def test_image_trainer_compute_eval_metrics(dev, tmp_path):
    """dSprites: the reference's key set next to the checkpoint, the values of the suite on its own representations with the
    same seed, and JSON null where a metric is not finite (a constant attribute: SAP divides by its zero variance)"""
    from arvae_amd.data import DspritesDataset
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    x, lab = syn.dsprites_batch(600, seed=3)
    lab[:, 1] = 2.0                                                  # 'shape' constant
    path = str(tmp_path / 'dsprites.npz')
    np.savez(path, imgs=(x[:, 0] > 0.5).astype(np.uint8), latents_values=lab.astype(np.float64))
    torch.manual_seed(0)
    model = DspritesVAE()
    trainer = ImageVAETrainer(DspritesDataset(path, device=dev), model, reg_type=('all',), reg_dim=(1, 2, 3, 4, 5))
    trainer.cuda()
    model.filepath = str(tmp_path / 'models' / 'd' / 'd.pt')
    metrics = trainer.compute_eval_metrics(batch_size=16, random_state=9)
    on_disk = _check_results(trainer, metrics, str(tmp_path / 'models' / 'd'), 9)
    assert on_disk['SAP_score'] is None and 'null' in open(tmp_path / 'models' / 'd' / 'results_dict.json').read()
    assert on_disk['interpretability']['shape'][1] == 1.0
    assert trainer.compute_eval_metrics(batch_size=16) == on_disk                     # loaded, not recomputed


def test_measure_trainer_compute_eval_metrics(dev, tmp_path):
    from arvae_amd.data import FolkNBarDataset
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=2)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    ds = FolkNBarDataset(dataset_dir=str(raw), device=dev)
    torch.manual_seed(0)
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.5, 16, 2, 64, 0.5, False, 'folk')
    trainer = MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))
    trainer.cuda()
    model.filepath = str(tmp_path / 'models' / 'm' / 'm.pt')
    metrics = trainer.compute_eval_metrics(batch_size=8, random_state=4)
    _check_results(trainer, metrics, str(tmp_path / 'models' / 'm'), 4)
    assert list(metrics['interpretability']) == ['rhy_complexity', 'pitch_range', 'note_density', 'contour', 'mean']


def _run_cli(script, args, env_dir):
    env = dict(os.environ, ARVAE_DATA_DIR=str(env_dir), ARVAE_MODEL_DIR=str(env_dir / 'models'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, timeout=600, env=env,
                       cwd=str(env_dir))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    start = r.stdout.index('{\n')
    return json.JSONDecoder().raw_decode(r.stdout[start:])[0]


def test_cli_metrics_flag(dev, tmp_path):
    """--metrics adds the reference's keys to the printed summary of both CLIs; without it the summary keeps its keys"""
    x, lab = syn.dsprites_batch(400, seed=0)
    np.savez(str(tmp_path / 'dsprites_ndarray_co1sh3sc6or40x32y32_64x64.npz'), imgs=(x[:, 0] > 0.5).astype(np.uint8),
             latents_values=lab.astype(np.float64))
    args = ['-d', 'dsprites', '--num_epochs', '1', '--batch_size', '64', '--rand', '3', '-r', 'all']
    plain = _run_cli('train_image_vae.py', args, tmp_path)
    assert not REFERENCE_KEYS & set(plain)
    with_metrics = _run_cli('train_image_vae.py', ['-d', 'dsprites', '--test', '--rand', '3', '-r', 'all', '--metrics'], tmp_path)
    assert REFERENCE_KEYS <= set(with_metrics) and set(plain) <= set(with_metrics)
    assert set(with_metrics['interpretability']) == set(with_metrics['attributes']) | {'mean'}
    raw = tmp_path / 'folk_raw_data'
    raw.mkdir()
    score = torch.from_numpy(syn.measure_batch(400, seed=0)).int()
    torch.save(torch.utils.data.TensorDataset(score, score), str(raw / '4by4_FolkNBarDataset_1_train'))
    i2n, n2i = syn.measure_vocabulary()
    (raw / 'index_dicts.txt').write_text(repr(i2n) + '\n' + repr(n2i) + '\n')
    summary = _run_cli('train_measure_vae.py', ['--num_epochs', '1', '--batch_size', '16', '--rand', '1', '-r', 'all', '--metrics'],
                       tmp_path)
    assert REFERENCE_KEYS <= set(summary) and summary['num_codes'] == 16

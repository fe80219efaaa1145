"""Host side of the disentanglement metrics (arvae_amd.evaluation): the reductions and the Spearman p-value against the
reference's recorded results (tests/golden/eval_metrics_*.npz, written by make_eval_goldens.py), the KSG entry points'
argument checks, and sklearn's preprocessing restated draw for draw.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import arvae_amd  # noqa: F401
from arvae_amd import evaluation as ev
from arvae_amd import synthetic as syn

KINDS = ('small', 'dsprites', 'mnist', 'measure')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(golden_dir, kind):
    return np.load(os.path.join(golden_dir, f'eval_metrics_{kind}.npz'))


def brute_force_ksg(x, y, k, digamma=None):
    """sklearn's _compute_mi_cc restated with dense NumPy fp64: (mi, radius, nx, ny).  digamma: a float digamma (scipy's, to
    reproduce sklearn's last bit); by default psi of an integer as a harmonic number"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.size
    dx = np.abs(x[None, :] - x[:, None])
    dy = np.abs(y[None, :] - y[:, None])
    d = np.maximum(dx, dy)
    np.fill_diagonal(d, np.inf)                                      # the query point is excluded by index
    r = np.nextafter(np.sort(d, axis=1)[:, k - 1], 0)
    nx = (dx <= r[:, None]).sum(1) - 1
    ny = (dy <= r[:, None]).sum(1) - 1

    def psi(m):                                                      # digamma of integers >= 1
        if digamma is not None:
            return digamma(np.asarray(m, np.float64))
        h = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, n + 1))])
        return h[np.asarray(m) - 1] - 0.57721566490153286061
    mi = psi(n) + psi(k) - np.mean(psi(nx + 1)) - np.mean(psi(ny + 1))
    return max(0.0, mi), r, nx, ny


@pytest.mark.parametrize('kind', KINDS)
def test_reductions_reproduce_the_reference_scalars(golden_dir, kind):
    g = golden(golden_dir, kind)
    interp_mean, corr, modularity, mig, sap = g['scalars']
    assert abs(np.mean(g['interp'][:, 1]) - interp_mean) <= 1e-12
    assert abs(ev.corr_score_from(g['scc']) - corr) <= 1e-12
    assert abs(ev.modularity_from(g['mi_mod'].T) - modularity) <= 1e-12
    assert abs(ev.mig_from(g['mi_mig'].T, g['entropy']) - mig) <= 1e-12
    assert abs(ev.sap_from(g['sap']) - sap) <= 1e-12
    names = [f'attr{a}' for a in range(g['interp'].shape[0])]
    # interpretability picks the first maximum of each call's MI vector
    r2 = np.zeros_like(g['sap'])
    for a, (dim, score) in enumerate(g['interp']):
        r2[int(dim), a] = score
    got = ev.interpretability_from(g['mi_interp'], r2, names)
    assert [got[n][0] for n in names] == [int(d) for d in g['interp'][:, 0]]
    assert abs(got['mean'][1] - interp_mean) <= 1e-12


@pytest.mark.parametrize('kind', KINDS)
def test_spearman_pvalue_matches_the_reference_decisions(golden_dir, kind):
    g = golden(golden_dir, kind)
    n = syn.EVAL_SHAPES[kind][0]
    rho, p = g['scc_rho'], g['scc_p']
    ours = np.vectorize(lambda r: ev.spearman_pvalue(float(r), n))(rho)
    assert np.array_equal(ours <= 0.05, p <= 0.05)
    big = p > 1e-200                                                 # below that both are 0 or denormal-ish
    np.testing.assert_allclose(ours[big], p[big], rtol=1e-8)
    np.testing.assert_array_equal(ev._scc_matrix(rho, n), g['scc'])


def test_betainc_edges():
    assert ev.betainc(2.0, 3.0, 0.0) == 0.0 and ev.betainc(2.0, 3.0, 1.0) == 1.0
    # I_x(1, 1) = x, I_x(a, 1) = x^a, I_x(1, b) = 1 - (1 - x)^b
    for x in (0.1, 0.5, 0.93):
        assert ev.betainc(1.0, 1.0, x) == pytest.approx(x, rel=1e-14)
        assert ev.betainc(3.5, 1.0, x) == pytest.approx(x ** 3.5, rel=1e-13)
        assert ev.betainc(1.0, 2.5, x) == pytest.approx(1 - (1 - x) ** 2.5, rel=1e-13)
    assert ev.spearman_pvalue(1.0, 100) == 0.0 and np.isnan(ev.spearman_pvalue(float('nan'), 100))
    assert ev.spearman_pvalue(0.0, 100) == pytest.approx(1.0, abs=1e-15)


def test_json_ready_writes_null_for_non_finite():
    got = ev.json_ready({'mig': float('nan'), 'x': np.float64(np.inf), 'i': {'a': (np.int64(3), np.float32(0.5))}, 's': 'k'})
    assert got == {'mig': None, 'x': None, 'i': {'a': [3, 0.5]}, 's': 'k'}


def test_ksg_entry_points_reject_bad_arguments():
    """the new ABI entry rejects bad arguments before any launch (pure host code)"""
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    lib = _lib.load()
    fake = ctypes.c_void_p(256)                                      # never dereferenced: every call below is refused first
    assert lib.arvae_ksg_ws_bytes(1000, 4) == 4 * 4 * 8
    assert lib.arvae_ksg_ws_bytes(0, 4) == -1 and lib.arvae_ksg_ws_bytes(10, 0) == -1
    ok = dict(x=fake, ldx=100, p=4, y=fake, n=100, k=3, ws=fake, mi=fake)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.arvae_ksg_mi(a['x'], a['ldx'], a['p'], a['y'], a['n'], a['k'], a['ws'], a['mi'], None, None, None, None)
    assert call(p=0) == -1 and b'p = 0' in lib.arvae_last_error_string()
    assert call(n=3) == -1 and b'n = 3' in lib.arvae_last_error_string()
    assert call(n=2) == -1
    assert call(k=9) == -1 and b'k = 9' in lib.arvae_last_error_string()
    assert call(k=0) == -1
    assert call(y=None) == -1 and b'null' in lib.arvae_last_error_string()
    assert call(x=None) == -1 and call(ws=None) == -1 and call(mi=None) == -1
    assert call(ldx=99) == -1 and b'ldx' in lib.arvae_last_error_string()


def test_product_does_not_import_sklearn_or_scipy():
    src = open(os.path.join(ROOT, 'ar-vae_amd', 'evaluation.py')).read()
    assert not re.search(r'^\s*(from|import)\s+(sklearn|scipy)\b', src, flags=re.M)


def test_preprocessing_plus_brute_force_equals_sklearn():
    """prepare_inputs (sklearn's scaling and noise, draw for draw) followed by a dense restatement of the KSG rules gives
    mutual_info_regression's numbers exactly: a three-level attribute, one with exact zeros (float32 noise case), a continuous
    one, the entropy case (an attribute against itself), y in float32 and float64"""
    sk = pytest.importorskip('sklearn.feature_selection')
    from scipy.special import digamma                                # (sklearn depends on scipy)
    codes, attrs, _ = syn.eval_metric_inputs('small', 0)
    for a in range(attrs.shape[1]):
        for y in (attrs[:, a], attrs[:, a].astype(np.float64)):
            for X, seed in ((codes, 3 + a), (attrs[:, a:a + 1], 11 + a)):
                want = sk.mutual_info_regression(X, y, random_state=seed)
                Xp, yp = ev.prepare_inputs(X, y, np.random.RandomState(seed))
                assert yp.dtype == y.dtype
                got = np.array([brute_force_ksg(Xp[:, c], yp, 3, digamma)[0] for c in range(Xp.shape[1])])
                np.testing.assert_array_equal(got, want)


def test_tiny_evaluation_split_leaves_the_metrics_out():
    """N <= n_neighbors: no KSG estimate exists; the trainers' entry warns and returns no keys (nothing reaches the device)"""
    codes, attrs, names = syn.eval_metric_inputs('small', 0)
    with pytest.warns(UserWarning, match='3 evaluation points'):
        assert ev.eval_metrics_or_warn(codes[:3], attrs[:3], names) == {}

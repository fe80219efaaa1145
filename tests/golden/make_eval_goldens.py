#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics_<kind>.npz by RUNNING THE REFERENCE's metric suite (utils/evaluation.py).

Build container only (needs the reference checkout, scikit-learn and scipy; none of them travel to the GPU box):

    python tests/golden/make_eval_goldens.py [/path/to/reference]

utils/evaluation.py is imported unmodified.  Its module-level `mutual_info_regression` is replaced by a wrapper that
pins `random_state = SEED + c` for the c-th call (and records the result), so that
arvae_amd.evaluation.compute_disentanglement_metrics(..., random_state=SEED) draws the same noise call for call.  The
inputs come from arvae_amd.synthetic.eval_metric_inputs(kind, 0); only outputs are stored:

  mi_interp / mi_mod / mi_mig  (A, z)  the MI vector of every KSG call of interpretability, modularity and MIG
  entropy                      (A,)    MIG's continuous_entropy calls
  scc, scc_rho, scc_p          (z, A)  Corr_score's matrix, and scipy's Spearman rho / p behind it
  sap                          (z, A)  SAP's score matrix
  interp                       (A, 2)  interpretability (dim, score) per attribute
  scalars                      (5,)    interpretability mean, Corr_score, modularity_score, mig, SAP_score
"""
import importlib.util
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ARVAE_REFERENCE', '/root/reference')
SEED = 17
KINDS = ('small', 'dsprites', 'mnist', 'measure')
SCALARS = ('interpretability', 'Corr_score', 'modularity_score', 'mig', 'SAP_score')


def load_reference_evaluation():
    spec = importlib.util.spec_from_file_location('ref_evaluation', os.path.join(REF, 'utils', 'evaluation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(kind):
    import scipy.stats
    import arvae_amd.synthetic as syn
    ev = load_reference_evaluation()
    inner = ev.mutual_info_regression
    calls = []

    def pinned(X, y, **kw):
        kw['random_state'] = SEED + len(calls)
        calls.append(inner(X, y, **kw))
        return calls[-1]
    ev.mutual_info_regression = pinned
    codes, attrs, names = syn.eval_metric_inputs(kind, 0)
    a = attrs.shape[1]
    interp = ev.compute_interpretability_metric(codes, attrs, names)
    metrics = {'interpretability': interp}
    metrics.update(ev.compute_correlation_score(codes, attrs))
    metrics.update(ev.compute_modularity(codes, attrs))
    metrics.update(ev.compute_mig(codes, attrs))
    metrics.update(ev.compute_sap_score(codes, attrs))
    assert len(calls) == 4 * a
    z = codes.shape[1]
    rho, p = np.zeros((z, a)), np.zeros((z, a))
    for i in range(z):
        for j in range(a):
            rho[i, j], p[i, j] = scipy.stats.spearmanr(codes[:, i], attrs[:, j])
    out = dict(mi_interp=np.stack(calls[:a]), mi_mod=np.stack(calls[a:2 * a]), mi_mig=np.stack(calls[2 * a:3 * a]),
               entropy=np.concatenate(calls[3 * a:]), scc=ev._compute_correlation_matrix(codes, attrs), scc_rho=rho, scc_p=p,
               sap=ev._compute_score_matrix(codes, attrs), interp=np.array([interp[n] for n in names], np.float64),
               scalars=np.array([interp['mean'][1]] + [float(metrics[k]) for k in SCALARS[1:]]), seed=np.int64(SEED))
    np.savez(os.path.join(HERE, f'eval_metrics_{kind}.npz'), **out)
    return kind, out['scalars']


if __name__ == '__main__':
    with Pool(len(KINDS)) as pool:
        for kind, scalars in pool.imap_unordered(run, KINDS):
            print(kind, dict(zip(SCALARS, scalars.round(6))), flush=True)

"""Disentanglement metrics of AR-VAE on the GPU: a drop-in for the reference's utils/evaluation.py.

Same public names and semantics: Interpretability, MIG, Modularity, SAP and SCC (Corr_score), plus
``compute_disentanglement_metrics`` that makes the reference's calls in the reference's order.  Depends on NumPy and torch
only; scikit-learn and scipy are not imported.

The expensive part, sklearn's KSG estimator (``mutual_info_regression``), runs on the device (csrc/ksg.hip).  Its host half --
sklearn's scaling and tie-breaking noise -- is restated here draw for draw, so that with the same ``random_state`` the
device sees the very points sklearn's neighbour searches see:
  * X: float64, each column divided by its np.nanstd (below 10 eps: 1), + 1e-10 * max(1, mean|X|) * N(0, 1) noise;
  * y keeps its dtype (float32 in every workload: attribute labels): scaled and noised in that dtype, drawn after X.
``random_state``: None draws from NumPy's global RandomState as sklearn does; a RandomState instance is used for every call; an
int s gives the c-th KSG call of the function ``RandomState(s + c)`` (goldens pin that).

Moments (SAP, the interpretability R^2) and Spearman ranks (SCC) are fp64 torch ops on the device; the Student-t p-value of
SCC is an fp64 regularised incomplete beta on the host.  Every function issues one device->host copy, at its end.
"""
import math
import warnings

import numpy as np
import torch

from . import _lib

EVAL_METRIC_DICT = {
    'interpretability': 'Interpretability',
    'modularity_score': 'Modularity',
    'mig': 'MIG',
    'SAP_score': 'SAP',
    'Corr_score': 'SCC',
}
METRIC_KEYS = ('interpretability', 'Corr_score', 'modularity_score', 'mig', 'SAP_score')


# ------------------------------------------------------------------------------------------------
# device KSG
# ------------------------------------------------------------------------------------------------
def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError('arvae_amd.evaluation runs its KSG estimator on the GPU (HIP kernel, no CPU fallback): no device visible')
    return torch.device('cuda', torch.cuda.current_device())


def _ptr(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ksg_mi(x_cols, y, n_neighbors=3, with_details=False):
    """KSG mutual information of each row of x_cols (p, n) with y (n,), both fp64 on the device.  -> mi (p,) on the device;
    with_details also the radii (p, n) fp64 and the marginal counts nx, ny (p, n) int32.  Enqueued only: nothing synchronises."""
    import ctypes
    if not (x_cols.is_cuda and y.is_cuda):
        raise RuntimeError('ksg_mi runs on the GPU only (HIP kernel, no CPU fallback)')
    if x_cols.dtype != torch.float64 or y.dtype != torch.float64:
        raise TypeError('ksg_mi needs fp64 columns')
    x_cols, y = x_cols.contiguous(), y.contiguous()
    p, n = x_cols.shape
    lib = _lib.load()
    ws_bytes = lib.arvae_ksg_ws_bytes(n, p)
    if ws_bytes < 0:
        _lib.check(ws_bytes, 'ksg_ws_bytes')
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=x_cols.device)
    mi = torch.empty(p, dtype=torch.float64, device=x_cols.device)
    radius = nx = ny = None
    if with_details:
        radius = torch.empty((p, n), dtype=torch.float64, device=x_cols.device)
        nx = torch.empty((p, n), dtype=torch.int32, device=x_cols.device)
        ny = torch.empty((p, n), dtype=torch.int32, device=x_cols.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x_cols.device).cuda_stream)
    _lib.check(lib.arvae_ksg_mi(_ptr(x_cols), n, p, _ptr(y), n, int(n_neighbors), _ptr(ws), _ptr(mi), _ptr(radius), _ptr(nx),
                                _ptr(ny), stream), 'ksg_mi')
    return (mi, radius, nx, ny) if with_details else mi


class _Draws:
    """The RandomState of each successive KSG call (see the module docstring)."""

    def __init__(self, random_state):
        self.random_state, self.calls = random_state, 0

    def next(self):
        rs = self.random_state
        self.calls += 1
        if rs is None:
            return np.random.mtrand._rand
        if isinstance(rs, np.random.RandomState):
            return rs
        return np.random.RandomState(int(rs) + self.calls - 1)


def prepare_inputs(X, y, rng):
    """sklearn's _estimate_mi preprocessing for dense continuous features: -> (X (n, p) float64, y (n,) in y's float dtype)."""
    X = np.asarray(X)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    y = np.asarray(y).reshape(-1)
    n = X.shape[0]
    if y.shape[0] != n:
        raise ValueError(f'X has {n} rows, y has {y.shape[0]}')
    X = X.astype(np.float64)
    cols = X[:, np.ones(X.shape[1], bool)]                 # the same copy sklearn scales (its continuous-feature mask)
    scale = np.nanstd(cols, axis=0)
    scale[scale < 10 * np.finfo(scale.dtype).eps] = 1.0
    cols /= scale
    X[:, :] = cols
    means = np.maximum(1, np.mean(np.abs(X[:, np.ones(X.shape[1], bool)]), axis=0))
    X += 1e-10 * means * rng.standard_normal(size=(n, X.shape[1]))
    if y.dtype not in (np.float32, np.float64):
        y = y.astype(np.float64)
    y = y.copy()
    s = np.nanstd(y, axis=0)                               # a scalar: only an exact 0 becomes 1 (sklearn's 1-D case)
    if s == 0.0:
        s = 1.0
    y /= s
    y += 1e-10 * np.maximum(1, np.mean(np.abs(y))) * rng.standard_normal(size=n)
    return X, y


def _upload(a, dev):
    """host array -> device tensor, copied from pinned memory without waiting for the stream (the host prepares the next KSG
    call while the device runs this one)"""
    host = torch.from_numpy(np.ascontiguousarray(a))
    if dev.type == 'cuda':
        host = host.pin_memory()
    return host.to(dev, non_blocking=True)


def _mi_device(X, y, rng, n_neighbors, dev):
    X, y = prepare_inputs(X, y, rng)
    if X.shape[0] <= n_neighbors:
        raise ValueError(f'KSG needs more than n_neighbors = {n_neighbors} points, got {X.shape[0]}')
    return ksg_mi(_upload(X, dev).t().contiguous(), _upload(y.astype(np.float64), dev), n_neighbors)


def mutual_info_regression(X, y, n_neighbors=3, random_state=None, device=None):
    """sklearn.feature_selection.mutual_info_regression for dense continuous X and continuous y, on the device.  -> (p,)"""
    return _mi_device(X, y, _Draws(random_state).next(), n_neighbors, _device(device)).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# the reference's MI helpers (utils/evaluation.py)
# ------------------------------------------------------------------------------------------------
def _mi_matrix(mus, ys, draws, dev, n_neighbors=3):
    """-> device (A, z): row a is the KSG call of attribute a against every code"""
    return torch.stack([_mi_device(mus, ys[:, a], draws.next(), n_neighbors, dev) for a in range(ys.shape[1])])


def _entropies(ys, draws, dev, n_neighbors=3):
    return torch.cat([_mi_device(ys[:, a].reshape(-1, 1), ys[:, a], draws.next(), n_neighbors, dev) for a in range(ys.shape[1])])


def continuous_mutual_info(mus, ys, random_state=None, device=None):
    """(num_codes, num_attributes) KSG mutual information of every code with every attribute"""
    return _mi_matrix(np.asarray(mus), np.asarray(ys), _Draws(random_state), _device(device)).t().cpu().numpy()


def continuous_entropy(ys, random_state=None, device=None):
    """(num_attributes,) KSG mutual information of each attribute with itself"""
    return _entropies(np.asarray(ys), _Draws(random_state), _device(device)).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# moments and ranks (device, fp64)
# ------------------------------------------------------------------------------------------------
def _columns(a, dev):
    """host (n, m) -> device (m, n) fp64, contiguous whatever the host layout (so the reductions' order, and their bits, do not
    depend on how the caller's array happens to be strided)"""
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev, torch.float64).t().contiguous()


def _centred(a, dev):
    t = _columns(a, dev)
    return t - t.mean(dim=1, keepdim=True)


def _cov_terms(mus_c, ys_c):
    """-> (cross (z, A), var_mu (z,), var_y (A,)) with ddof = 1, as np.cov"""
    n = mus_c.shape[1]
    cross = (mus_c[:, None, :] * ys_c[None, :, :]).sum(-1) / (n - 1)
    return cross, (mus_c * mus_c).sum(-1) / (n - 1), (ys_c * ys_c).sum(-1) / (n - 1)


def _average_ranks(cols):
    """scipy.stats.rankdata(method='average') of each row of cols (m, n), 1-based, fp64"""
    m, n = cols.shape
    s, order = torch.sort(cols, dim=1, stable=True)
    new = torch.ones_like(s, dtype=torch.bool)
    new[:, 1:] = s[:, 1:] != s[:, :-1]
    group = torch.cumsum(new.to(torch.int64), dim=1) - 1
    pos = torch.arange(n, device=cols.device, dtype=torch.int64).expand(m, n)
    first = torch.full((m, n), n, device=cols.device, dtype=torch.int64).scatter_reduce(1, group, pos, 'amin')
    last = torch.full((m, n), -1, device=cols.device, dtype=torch.int64).scatter_reduce(1, group, pos, 'amax')
    avg = (first.gather(1, group) + last.gather(1, group)).to(torch.float64) * 0.5 + 1.0
    return torch.empty_like(avg).scatter_(1, order, avg)


def _spearman_rho(mus, ys, dev):
    """(z, A) Spearman rho on average ranks (NaN where a column is constant, as scipy)"""
    rm, ra = _average_ranks(_columns(mus, dev)), _average_ranks(_columns(ys, dev))
    rm, ra = rm - rm.mean(1, keepdim=True), ra - ra.mean(1, keepdim=True)
    num = (rm[:, None, :] * ra[None, :, :]).sum(-1)
    rho = num / torch.sqrt((rm * rm).sum(-1)[:, None] * (ra * ra).sum(-1)[None, :])
    return rho.clamp(-1.0, 1.0)


def _pearson_sq(mus, ys, dev):
    """-> (r^2 (z, A), var_mu (z,)): the squared Pearson correlation of every pair, fp64"""
    cross, var_mu, var_y = _cov_terms(_centred(mus, dev), _centred(ys, dev))
    return cross * cross / (var_mu[:, None] * var_y[None, :]), var_mu


# ------------------------------------------------------------------------------------------------
# Student t p-value (host, fp64)
# ------------------------------------------------------------------------------------------------
def _betacf(a, b, x):
    """continued fraction of the incomplete beta function (modified Lentz)"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + aa / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h


def betainc(a, b, x, xc=None):
    """regularised incomplete beta I_x(a, b) in fp64; xc = 1 - x when the caller has it without cancellation"""
    xc = 1.0 - x if xc is None else xc
    if not (x == x):
        return math.nan
    if x <= 0.0:
        return 0.0
    if xc <= 0.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(xc))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, xc) / b


def spearman_pvalue(rho, n):
    """two-sided p of scipy.stats.spearmanr: t = rho sqrt(dof / ((1 + rho)(1 - rho))), dof = n - 2, Student t"""
    if not (rho == rho):
        return math.nan
    dof = n - 2.0
    den = (rho + 1.0) * (1.0 - rho)
    t2 = math.inf if den <= 0.0 else rho * rho * max(dof / den, 0.0)
    if t2 == math.inf:
        return 0.0
    return betainc(0.5 * dof, 0.5, dof / (dof + t2), t2 / (dof + t2))


def _scc_matrix(rho, n):
    """|rho| where p <= 0.05, else 0 (NaN rho -> 0)"""
    out = np.zeros_like(rho)
    for idx, r in np.ndenumerate(rho):
        if spearman_pvalue(float(r), n) <= 0.05:
            out[idx] = abs(r)
    return out


# ------------------------------------------------------------------------------------------------
# reductions (host, NumPy: the matrices are z x A)
# ------------------------------------------------------------------------------------------------
def interpretability_from(mi_rows, r2, attr_list):
    """mi_rows (A, z): one KSG call per attribute; r2 (z, A) -> {attr: (dim, score), 'mean': (-1, mean)}"""
    out, total = {}, 0.0
    for a, name in enumerate(attr_list):
        dim = int(np.argmax(mi_rows[a]))
        score = float(r2[dim, a])
        out[name] = (dim, score)
        total += score
    out['mean'] = (-1, total / len(attr_list))
    return out


def modularity_from(mi):
    """mi (z, A) -> mean over codes of 1 - (sum - max) / (max (A - 1)) of the squared MI, 0 where the max is 0"""
    sq = np.square(mi)
    top = np.max(sq, axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        score = 1.0 - (np.sum(sq, axis=1) - top) / (top * (sq.shape[1] - 1.0))
    score[top == 0.0] = 0.0
    return float(np.mean(score))


def mig_from(mi, entropy):
    """mi (z, A), entropy (A,) -> mean over attributes of the top-two MI gap over the entropy"""
    ranked = np.sort(mi, axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.mean((ranked[-1, :] - ranked[-2, :]) / entropy))


def corr_score_from(scc):
    return float(np.mean(np.max(scc, axis=0)))


def sap_matrix_from(r2, var_mu):
    return np.where(var_mu[:, None] > 1e-12, r2, 0.0)


def sap_from(sap):
    ranked = np.sort(sap, axis=0)
    return float(np.mean(ranked[-1, :] - ranked[-2, :]))


def _r2_for_interpretability(r2, var_y_zero):
    # the reference's LinearRegression R^2: a constant code explains nothing (0); a constant attribute is fitted exactly (1)
    r2 = np.where(np.isnan(r2), 0.0, r2)
    r2[:, var_y_zero] = 1.0
    return r2


# ------------------------------------------------------------------------------------------------
# the reference's public metric functions
# ------------------------------------------------------------------------------------------------
def _host(*tensors):
    """ONE device->host copy for the tensors of a metric (flattened fp64, split again on the host)"""
    flat = torch.cat([t.reshape(-1).to(torch.float64) for t in tensors]).cpu().numpy()
    out, at = [], 0
    for t in tensors:
        out.append(flat[at:at + t.numel()].reshape(tuple(t.shape)))
        at += t.numel()
    return out


def compute_interpretability_metric(latent_codes, attributes, attr_list, random_state=None, device=None):
    dev = _device(device)
    mus, ys = np.asarray(latent_codes), np.asarray(attributes)
    mi = _mi_matrix(mus, ys, _Draws(random_state), dev)
    r2, _ = _pearson_sq(mus, ys, dev)
    mi, r2 = _host(mi, r2)
    return interpretability_from(mi, _r2_for_interpretability(r2, np.ptp(ys, axis=0) == 0), attr_list)


def compute_mig(latent_codes, attributes, random_state=None, device=None):
    dev = _device(device)
    draws = _Draws(random_state)
    mi = _mi_matrix(np.asarray(latent_codes), np.asarray(attributes), draws, dev)
    h = _entropies(np.asarray(attributes), draws, dev)
    mi, h = _host(mi, h)
    return {'mig': mig_from(mi.T, h)}


def compute_modularity(latent_codes, attributes, random_state=None, device=None):
    mi = continuous_mutual_info(latent_codes, attributes, random_state, device)
    return {'modularity_score': modularity_from(mi)}


def compute_correlation_score(latent_codes, attributes, device=None):
    rho, = _host(_spearman_rho(latent_codes, attributes, _device(device)))
    return {'Corr_score': corr_score_from(_scc_matrix(rho, np.asarray(latent_codes).shape[0]))}


def compute_sap_score(latent_codes, attributes, device=None):
    r2, var_mu = _host(*_pearson_sq(latent_codes, attributes, _device(device)))
    return {'SAP_score': sap_from(sap_matrix_from(r2, var_mu))}


def compute_disentanglement_metrics(latent_codes, attributes, attr_list, random_state=None, device=None, n_neighbors=3,
                                    return_details=False):
    """The reference's compute_eval_metrics suite in its order -- interpretability, SCC, modularity, MIG (MI matrix, then the
    entropies), SAP -- with one draw stream across the KSG calls (random_state s: the c-th call uses RandomState(s + c)).
    -> {'interpretability': {attr: (dim, score), 'mean': (-1, m)}, 'Corr_score', 'modularity_score', 'mig', 'SAP_score'};
    return_details adds the matrices behind them under '_details'.  One device->host copy in all."""
    dev = _device(device)
    mus, ys = np.asarray(latent_codes), np.asarray(attributes)
    if mus.ndim != 2 or ys.ndim != 2 or mus.shape[0] != ys.shape[0] or ys.shape[1] != len(attr_list):
        raise ValueError(f'latent codes {mus.shape}, attributes {ys.shape}, {len(attr_list)} names')
    draws = _Draws(random_state)
    mi_interp = _mi_matrix(mus, ys, draws, dev, n_neighbors)
    rho = _spearman_rho(mus, ys, dev)
    mi_mod = _mi_matrix(mus, ys, draws, dev, n_neighbors)
    mi_mig = _mi_matrix(mus, ys, draws, dev, n_neighbors)
    entropy = _entropies(ys, draws, dev, n_neighbors)
    r2, var_mu = _pearson_sq(mus, ys, dev)
    mi_interp, rho, mi_mod, mi_mig, entropy, r2, var_mu = _host(mi_interp, rho, mi_mod, mi_mig, entropy, r2, var_mu)
    scc = _scc_matrix(rho, mus.shape[0])
    sap = sap_matrix_from(r2, var_mu)
    metrics = {'interpretability': interpretability_from(mi_interp, _r2_for_interpretability(r2, np.ptp(ys, axis=0) == 0), attr_list),
               'Corr_score': corr_score_from(scc), 'modularity_score': modularity_from(mi_mod.T),
               'mig': mig_from(mi_mig.T, entropy), 'SAP_score': sap_from(sap)}
    if return_details:
        metrics['_details'] = dict(mi_interp=mi_interp, mi_mod=mi_mod, mi_mig=mi_mig, entropy=entropy, scc=scc, scc_rho=rho,
                                   sap=sap)
    return metrics


def json_ready(metrics):
    """metrics as plain JSON values: tuples -> lists, NumPy scalars -> float / int, non-finite -> None (JSON null: NaN != NaN
    would make a reloaded results file differ from itself)"""
    if isinstance(metrics, dict):
        return {k: json_ready(v) for k, v in metrics.items()}
    if isinstance(metrics, (list, tuple)):
        return [json_ready(v) for v in metrics]
    if isinstance(metrics, (int, np.integer)) and not isinstance(metrics, bool):
        return int(metrics)
    if isinstance(metrics, (float, np.floating)):
        return float(metrics) if math.isfinite(metrics) else None
    return metrics


def eval_metrics_or_warn(latent_codes, attributes, attr_list, random_state=None, n_neighbors=3):
    """the trainers' entry: the suite as JSON-ready values, or {} with a warning when the evaluation split has too few points
    for a k-nearest-neighbour estimate (N <= n_neighbors)"""
    n = np.asarray(latent_codes).shape[0]
    if n <= n_neighbors:
        warnings.warn(f'disentanglement metrics skipped: {n} evaluation points, the KSG estimator needs more than {n_neighbors}')
        return {}
    return json_ready(compute_disentanglement_metrics(latent_codes, attributes, attr_list, random_state=random_state,
                                                      n_neighbors=n_neighbors))

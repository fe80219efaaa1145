"""Cases, float64 / float32 restatement and row screening for the float64 bars of the latent block (ar-vae_amd/csrc/midcluster.hip,
midblock.hip): shared by test_latent_block_cases.py (CPU) and test_latent_block_float64.py (GPU).  No test and no GPU import in here.

Why the rows are screened.  One ReLU unit whose pre-activation changes sign between two fp32 summation orders moves the worst
per-parameter gradient error of ANY fp32 implementation from ~1e-6 to ~1e-3 relative L2, so a bar built on the error of the fp32 CPU
yardstick is a lottery while such units exist.  The forward pass never couples two batch rows, so rows can be chosen one by one: a
row is kept when every ReLU / SELU unit of that row has |pre64| >= tau * rms(layer), rms(layer) the root-mean-square of that layer's
float64 pre-activations over the pool and tau = TAU_FACTOR (16) times the largest |pre32 - pre64| / rms(layer) the fp32 CPU yardstick
shows anywhere in the pool.  That many units can be screened only while few layers have an activation, so the regimes below keep
the activations where the latent block needs them and make the other conv layers linear (the executor's own 32-channel fast paths
ask for a ReLU layer; the per-layer link kernels a linear layer takes instead carry float64 bars of their own:
test_conv32_links_float64.py, test_split_kernels_float64.py, test_single_channel_links_float64.py).

Regimes (per-layer activation lists; the executor reads them from the cached descriptor, FusedImageVAE.descriptor()):
  dsprites_block   ReLU on enc_conv.4, enc_conv.6, enc_lin.0/2, dec_lin.0/2/4 and dec_conv.0 (6144 units per row); enc_conv.0/2 and
                   dec_conv.2/4 linear.  What midc_fold_topology() asks for: the clustered kernels run WITH the two folded conv layers
                   (backward: the linear dec_conv.2 hands them an ungated gradient, which plan.hip then gates in one operand pass).
  mnist_block      SELU and its Dropout keep-mask on enc_conv.6 (the gate of the wide data-gradient GEMM), SELU on enc_lin.0 and
                   dec_lin.0/2 (6288 units per row); the other four hidden conv layers linear, their keep-masks stay.  Train mode.
  full             the models as they are (oracle.image_vae): for the bit-for-bit check of the restatement only.

Hyperparameters of every case: beta 4, gamma 10, delta 1, capacity 0, reg_dim (1..5) / (1..6), weights synth_state(SHAPES[kind],
seed, GAIN[kind]) with seed 9, GAIN 1.6 (dSprites) and 0.7 (Morpho-MNIST; the float64 logits of the mnist_block regime have rms
0.127 .. 0.129 at the four batches, inside the [0.02, 8] outside of which the gain was to be changed).

Batches, each for an edge of the code:
  dSprites clustered (32 rows and 16 member workgroups per cluster)   1, 33 (second cluster with one row), 72 (three clusters, the
      last with 8 rows, no multiple of the 8 XCDs), 259 (nine clusters: one more than the XCDs, the last with 3 rows)
  dSprites rows (no_cluster)   1, 33 (one row per workgroup), 259 (two, the last workgroup has one), 515 (four, the last has three)
  Morpho-MNIST (row kernel + 64 x 64 tile GEMMs)   1, 3, 47, 67
"""
import functools
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from arvae_amd import synthetic as syn
from oracle import image_vae as o_vae

from split_cases import FLOOR, R          # noqa: F401  (the bar: e <= R * e_cpu + FLOOR)

TAU_FACTOR = 16.0
POOL_FACTOR = 6
BETA, GAMMA, DELTA, CAPACITY = 4.0, 10.0, 1.0, 0.0
GAIN = {'dsprites': 1.6, 'mnist': 0.7}
REG_DIMS = {'dsprites': (1, 2, 3, 4, 5), 'mnist': (1, 2, 3, 4, 5, 6)}
WEIGHT_SEED = 9
E_CPU_CEILING = 1.0e-4                     # sanity ceiling on the yardstick's own gradient error: a flip that slipped through shows above it

CLUSTER_BATCHES = (1, 33, 72, 259)
ROWS_BATCHES = (1, 33, 259, 515)
MNIST_BATCHES = (1, 3, 47, 67)
CASES = [('dsprites', b) for b in sorted(set(CLUSTER_BATCHES + ROWS_BATCHES))] + [('mnist', b) for b in MNIST_BATCHES]
REGIME_OF = {'dsprites': 'dsprites_block', 'mnist': 'mnist_block'}
# the Morpho-MNIST-shaped model at other hidden widths (kind, batch, width): 40 and 52 are no multiples of the tile GEMMs' 32-wide
# chunk.  At 40 the bf16 planes of a 2888-wide matrix (both axes padded to 32) do not fit the space of the fp32 layouts they would
# replace, which alone keeps the layer on the row kernels; at 52 they fit, and only the fits check of mid_describe() keeps it there
WIDTH_CASES = [('mnist', 5, 40), ('mnist', 5, 52), ('mnist', 5, 32), ('mnist', 5, 64)]

# ---- layer tables: (name, op, activation in the full model, dropout mask index or None), in execution order
_DS_ENC = [('enc_conv.0', 'conv', 'relu', None), ('enc_conv.2', 'conv', 'relu', None), ('enc_conv.4', 'conv', 'relu', None),
           ('enc_conv.6', 'conv', 'relu', None), ('enc_lin.0', 'lin', 'relu', None), ('enc_lin.2', 'lin', 'relu', None)]
_DS_DEC = [('dec_lin.0', 'lin', 'relu', None), ('dec_lin.2', 'lin', 'relu', None), ('dec_lin.4', 'lin', 'relu', None),
           ('dec_conv.0', 'deconv', 'relu', None), ('dec_conv.2', 'deconv', 'relu', None), ('dec_conv.4', 'deconv', 'relu', None),
           ('dec_conv.6', 'deconv', 'none', None)]
_MN_ENC = [('enc_conv.0', 'conv', 'selu', 0), ('enc_conv.3', 'conv', 'selu', 1), ('enc_conv.6', 'conv', 'selu', 2),
           ('enc_lin.0', 'lin', 'selu', None)]
_MN_DEC = [('dec_lin.0', 'lin', 'selu', None), ('dec_lin.2', 'lin', 'selu', None), ('dec_conv.0', 'deconv', 'selu', 3),
           ('dec_conv.3', 'deconv', 'selu', 4), ('dec_conv.6', 'deconv', 'none', None)]
LAYERS = {'dsprites': (_DS_ENC, _DS_DEC), 'mnist': (_MN_ENC, _MN_DEC)}
_CONV_GEOM = {'dsprites': dict(stride=2, padding=1), 'mnist': dict(stride=1, padding=0)}
_DEC_GRID = {'dsprites': (32, 4, 4), 'mnist': (8, 19, 19)}

_ACTIVE = {
    'dsprites_block': ('enc_conv.4', 'enc_conv.6', 'enc_lin.0', 'enc_lin.2', 'dec_lin.0', 'dec_lin.2', 'dec_lin.4', 'dec_conv.0'),
    'mnist_block': ('enc_conv.6', 'enc_lin.0', 'dec_lin.0', 'dec_lin.2'),
}


def acts(kind, regime):
    """-> (encoder list, decoder list) of 'none' / 'relu' / 'selu', one entry per layer in execution order (heads not included)"""
    enc, dec = LAYERS[kind]
    if regime == 'full':
        return [l[2] for l in enc], [l[2] for l in dec]
    on = _ACTIVE[regime]
    return [l[2] if l[0] in on else 'none' for l in enc], [l[2] if l[0] in on else 'none' for l in dec]


def _act(pre, act):
    return F.relu(pre) if act == 'relu' else o_vae.selu(pre) if act == 'selu' else pre


def _dact(pre, act):
    """d act / d pre, or None for the identity"""
    if act == 'relu':
        return (pre > 0).to(pre.dtype)
    if act == 'selu':
        return o_vae.SELU_SCALE * torch.where(pre > 0, torch.ones_like(pre), o_vae.SELU_ALPHA * torch.exp(pre))
    return None


def _apply(kind, op, h, w, b):
    if op == 'conv':
        return F.conv2d(h, w, b, **_CONV_GEOM[kind])
    if op == 'deconv':
        return F.conv_transpose2d(h, w, b, **_CONV_GEOM[kind])
    return F.linear(h, w, b)


def forward(kind, regime, p, x, eps, masks, mutate=None, stop_after_last_act=False):
    """The forward pass layer by layer, in the operations and the order of oracle.image_vae.forward (regime 'full' in float32 is that
    function bit for bit).  p: {key: tensor}; everything in p's dtype.  mutate: {layer name: f(pre) -> pre} applied to a layer's
    pre-activation (the fault injected by the separation test).  -> dict(logits, mu, log_std, sigma, z, pre {layer: pre-activation of
    every layer that has an activation}, tape [(name, op, act, mask, input, pre)] for backward())"""
    enc, dec = LAYERS[kind]
    a_enc, a_dec = acts(kind, regime)
    b = x.shape[0]
    tape, pre_of = [], OrderedDict()
    last_active = max([i for i, a in enumerate(a_dec) if a != 'none'], default=-1)

    def run(layer, act, h):
        name, op, _, mi = layer
        pre = _apply(kind, op, h, p[name + '.weight'], p[name + '.bias'])
        if mutate is not None and name in mutate:
            pre = mutate[name](pre)
        mask = None if (masks is None or mi is None) else masks[mi]
        out = o_vae._drop(_act(pre, act), mask)
        tape.append((name, op, act, mask, h, pre))
        if act != 'none':
            pre_of[name] = pre
        return out

    h = x
    for layer, act in zip(enc, a_enc):
        if layer[1] == 'lin' and h.dim() > 2:
            h = h.reshape(b, -1)
        h = run(layer, act, h)
    mu = F.linear(h, p['enc_mean.weight'], p['enc_mean.bias'])
    log_std = F.linear(h, p['enc_log_std.weight'], p['enc_log_std.bias'])
    sigma = torch.exp(log_std)
    z = mu + eps * sigma
    hidden = h
    h = z
    for i, (layer, act) in enumerate(zip(dec, a_dec)):
        if stop_after_last_act and i > last_active:
            h = None
            break
        if layer[1] == 'deconv' and h.dim() == 2:
            h = h.reshape((b,) + _DEC_GRID[kind])
        h = run(layer, act, h)
    return dict(logits=h, mu=mu, log_std=log_std, sigma=sigma, z=z, pre=pre_of, tape=tape, hidden=hidden)


def loss_terms(kind, fw, x, labels):
    """The oracle's formulas (oracle/losses.py) in the tensors' own dtype, with their closed-form gradients: -> (scalars dict,
    d loss / d logits, d / d mu, d / d log_std, d / d z) where the last three are the DIRECT terms (KL, regulariser)"""
    logits, mu, sigma, z = fw['logits'], fw['mu'], fw['sigma'], fw['z']
    b = x.shape[0]
    recon = (torch.clamp(logits, min=0) - logits * x + torch.log1p(torch.exp(-logits.abs()))).sum() / b
    d_logits = (torch.sigmoid(logits) - x) / b
    var = sigma * sigma
    kl = (0.5 * (var + mu * mu - 1.0 - torch.log(var))).sum(1).mean()
    dist = BETA * (kl - CAPACITY).abs()
    sgn = torch.sign(kl - CAPACITY)
    d_mu = BETA * sgn * mu / b
    d_ls = BETA * sgn * (var - 1.0) / b                       # d / d sigma = (sigma - 1 / sigma) / b, times d sigma / d log_std = sigma
    reg = z.new_zeros(())
    d_z = torch.zeros_like(z)
    for d in REG_DIMS[kind]:
        a, v = labels[:, d], z[:, d]
        t = torch.tanh(DELTA * (v[:, None] - v[None, :]))
        s = torch.sign(a[:, None] - a[None, :])
        reg = reg + GAMMA * (t - s).abs().mean()
        d_z[:, d] = (2.0 * GAMMA * DELTA / (b * b)) * ((1.0 - t * t) * torch.sign(t - s)).sum(1)
    acc = ((logits >= 0) == (x >= 0.5)).to(torch.float64).mean()
    scalars = dict(loss=float(recon + dist + reg), recon=float(recon), dist=float(dist), reg=float(reg), kl=float(kl), acc=float(acc))
    return scalars, d_logits, d_mu, d_ls, d_z


def backward(kind, p, fw, eps, d_logits, d_mu, d_ls, d_z):
    """Gradients of every parameter by hand (no autograd): the tape of forward() walked backwards"""
    grads = {}
    geom = _CONV_GEOM[kind]
    n_dec = len(LAYERS[kind][1])

    def back(entry, g):
        name, op, act, mask, h, pre = entry
        if mask is not None:
            g = g * mask.to(g.dtype).reshape(g.shape) * 2.0
        da = _dact(pre, act)
        if da is not None:
            g = g * da
        w = p[name + '.weight']
        if op == 'lin':
            grads[name + '.weight'] = g.t() @ h
            grads[name + '.bias'] = g.sum(0)
            return g @ w
        grads[name + '.bias'] = g.sum((0, 2, 3))
        if op == 'conv':
            grads[name + '.weight'] = torch.nn.grad.conv2d_weight(h, w.shape, g, **geom)
            return F.conv_transpose2d(g, w, None, **geom)
        # a transposed convolution is the adjoint of conv2d(., w): <convT(h, w), g> = <h, conv2d(g, w)>
        grads[name + '.weight'] = torch.nn.grad.conv2d_weight(g, w.shape, h, **geom)
        return F.conv2d(g, w, None, **geom)

    tape = fw['tape']
    g = d_logits
    for entry in reversed(tape[len(tape) - n_dec:]):
        g = back(entry, g.reshape(entry[5].shape))
    g_z = g + d_z
    g_mu = g_z + d_mu
    g_ls = g_z * eps * fw['sigma'] + d_ls
    hidden = fw['hidden']
    grads['enc_mean.weight'], grads['enc_mean.bias'] = g_mu.t() @ hidden, g_mu.sum(0)
    grads['enc_log_std.weight'], grads['enc_log_std.bias'] = g_ls.t() @ hidden, g_ls.sum(0)
    g = g_mu @ p['enc_mean.weight'] + g_ls @ p['enc_log_std.weight']
    for entry in reversed(tape[:len(tape) - n_dec]):
        g = back(entry, g.reshape(entry[5].shape))
    return grads


def _tensors(state, x, labels, eps, masks, dtype):
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in state.items()}
    xt, lt, et = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in (x, labels, eps))
    mt = None if masks is None else [torch.from_numpy(m) for m in masks]
    return p, xt, lt, et, mt


def step(kind, regime, state, x, labels, eps, masks, dtype, mutate=None):
    """One whole training step's forward and backward in `dtype` (torch.float64: the reference; torch.float32: the CPU yardstick):
    forward, reconstruction term, beta |KL - c|, the all-pairs regulariser, accuracy, every gradient.  numpy in, numpy (float64) out:
    dict(mu, sigma, z, logits, scalars {loss, recon, dist, reg, kl, acc}, grads {parameter name: array}, pre {layer: array})"""
    p, xt, lt, et, mt = _tensors(state, x, labels, eps, masks, dtype)
    with torch.no_grad():
        fw = forward(kind, regime, p, xt, et, mt, mutate=mutate)
        scalars, d_logits, d_mu, d_ls, d_z = loss_terms(kind, fw, xt, lt)
        grads = backward(kind, p, fw, et, d_logits, d_mu, d_ls, d_z)

    def out(t):
        return t.detach().to(torch.float64).numpy()
    return dict(mu=out(fw['mu']), sigma=out(fw['sigma']), z=out(fw['z']), logits=out(fw['logits']), scalars=scalars,
                grads={k: out(v) for k, v in grads.items()}, pre={k: out(v) for k, v in fw['pre'].items()})


def inputs(kind, n, seed):
    """x, labels, eps, masks of n rows: the project's synthetic batches, keyed by one seed"""
    x, lab = (syn.dsprites_batch if kind == 'dsprites' else syn.mnist_batch)(n, seed=seed)
    eps = syn.normal_noise((n, o_vae.Z_DIM[kind]), seed=seed + 1)
    masks = syn.dropout_masks([(n,) + s for s in o_vae.MNIST_MASK_SHAPES], seed + 2) if kind == 'mnist' else None
    return x, lab, eps, masks


def _pool_pre(kind, regime, state, x, eps, masks, dtype, chunk=256):
    """pre-activations of every active layer over the pool, in chunks of rows (no row talks to another in the forward pass)"""
    parts = {}
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in state.items()}
    with torch.no_grad():
        for lo in range(0, x.shape[0], chunk):
            sl = slice(lo, lo + chunk)
            mt = None if masks is None else [torch.from_numpy(m[sl]) for m in masks]
            fw = forward(kind, regime, p, torch.from_numpy(x[sl]).to(dtype), torch.from_numpy(eps[sl]).to(dtype), mt,
                         stop_after_last_act=True)
            for k, v in fw['pre'].items():
                parts.setdefault(k, []).append(v.reshape(v.shape[0], -1).to(torch.float64).numpy())
    return {k: np.concatenate(v) for k, v in parts.items()}


def seed_of(kind, batch):
    return (3000 if kind == 'dsprites' else 5000) + batch


def shapes(kind, width=None):
    """parameter shapes of the model; width: the Morpho-MNIST-shaped model with that hidden width instead of 256"""
    if width is None:
        return o_vae.SHAPES[kind]
    return OrderedDict((k, tuple(width if d == 256 else d for d in s)) for k, s in o_vae.SHAPES[kind].items())


@functools.lru_cache(maxsize=None)
def screened_batch(kind, regime, batch, seed, width=None):
    """A batch of `batch` rows none of whose ReLU / SELU units sits within tau * rms(layer) of zero (module docstring): the first
    `batch` passing rows of a pool of POOL_FACTOR * batch.  Raises when fewer pass: a condition of the tests, not a measurement.
    -> dict(state, x, labels, eps, masks, tau, pool, passed, pass_rate, yardstick (largest |pre32 - pre64| / rms), rms {layer})"""
    t0 = time.time()
    pool = POOL_FACTOR * batch
    state = syn.synth_state(shapes(kind, width), WEIGHT_SEED, GAIN[kind])
    x, lab, eps, masks = inputs(kind, pool, seed)
    pre64 = _pool_pre(kind, regime, state, x, eps, masks, torch.float64)
    pre32 = _pool_pre(kind, regime, state, x, eps, masks, torch.float32)
    rms = {k: float(np.sqrt(np.mean(v * v))) for k, v in pre64.items()}
    yard = max(float(np.abs(pre32[k] - pre64[k]).max()) / rms[k] for k in pre64)
    tau = TAU_FACTOR * yard
    margin = np.min([np.abs(v).min(1) / rms[k] for k, v in pre64.items()], axis=0)
    ok = np.flatnonzero(margin >= tau)
    print(f'screened_batch {kind} {regime}{"" if width is None else f" width {width}"} B={batch}: pool {pool}, yardstick {yard:.3e}, '
          f'tau {tau:.3e}, passed {ok.size} (rate {ok.size / pool:.2f}), {time.time() - t0:.1f} s')
    if ok.size < batch:
        raise RuntimeError(f'screened_batch({kind}, {regime}, {batch}, {seed}): only {ok.size} of {pool} rows pass tau = {tau:.3e}')
    keep = ok[:batch]
    return dict(state=state, x=np.ascontiguousarray(x[keep]), labels=np.ascontiguousarray(lab[keep]), eps=np.ascontiguousarray(eps[keep]),
                masks=None if masks is None else [np.ascontiguousarray(m[keep]) for m in masks], tau=tau, pool=pool, passed=int(ok.size),
                pass_rate=ok.size / pool, yardstick=yard, rms=rms)


@functools.lru_cache(maxsize=None)
def case(kind, batch, width=None):
    """The screened batch of (kind, batch) with its float64 reference and fp32 CPU yardstick (computed once per process; callers
    leave them unchanged): screened_batch()'s dict + ref, cpu (step() results)"""
    regime = REGIME_OF[kind]
    c = dict(screened_batch(kind, regime, batch, seed_of(kind, batch) + (width or 0), width))
    t0 = time.time()
    c['regime'] = regime
    c['ref'] = step(kind, regime, c['state'], c['x'], c['labels'], c['eps'], c['masks'], torch.float64)
    c['cpu'] = step(kind, regime, c['state'], c['x'], c['labels'], c['eps'], c['masks'], torch.float32)
    print(f'case {kind} B={batch}: float64 + fp32 CPU steps {time.time() - t0:.1f} s')
    return c


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def flips(a, b):
    """units whose pre-activation has a different sign in the two step() results"""
    return sum(int(((a['pre'][k] > 0) != (b['pre'][k] > 0)).sum()) for k in a['pre'])


def last_cluster_rows(batch, rows_per_cluster=32):
    lo = (batch - 1) // rows_per_cluster * rows_per_cluster
    return lo, batch


def drop_slice_mutation(batch, bias, col0=16 * 5, width=16):
    """the fault of the separation test, as {layer: f(pre)} for step(mutate=): one 16-column slice (one member workgroup's share of a
    256-wide layer) of enc_lin.2's PRODUCT zeroed for the rows of the last cluster -- the bias (numpy, [256]) stays, as it would in
    a kernel that skips the slice"""
    lo, hi = last_cluster_rows(batch)

    def f(pre):
        pre = pre.clone()
        pre[lo:hi, col0:col0 + width] = torch.from_numpy(bias[col0:col0 + width]).to(pre.dtype)
        return pre
    return {'enc_lin.2': f}

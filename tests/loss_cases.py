"""Case tables, float64 references, fp32 CPU yardsticks and the bar of the float64 accuracy tests of the loss-side kernels
(ar-vae_amd/csrc/losses.hip, regloss.h, recon_elem in common.h): latent head, beta-KL, all-pairs attribute regulariser, image and
token reconstruction terms, scale_by_scalar, Adam.  Shared by the GPU test (test_loss_kernels_float64.py) and by the CPU test that
proves the references right and the bar discriminating (test_loss_cases.py).  No test in here.

Per family:   <family>_CASES            the table (plain tuples; case_id(case) is the pytest id)
              <family>_inputs(case)     the fp32 inputs (numpy, seeded by the case's id) plus the case's parameters
              <family>_ref(inp)         float64 reference (numpy); takes the kernel's fp32 constants where it has any, so that it is
                                        the SAME operation
              <family>_cpu(inp)         the fp32 CPU yardstick (torch fp32, oracle.losses.adam_step, or for the regulariser an fp32
                                        numpy restatement of the kernel's documented formula with fp32 row sums)
              <family>_chain(inp, wrong)  the kernel's formula restated in plain fp32 numpy, sums in sequential chains (seq_rows): a worse
                                        order than a kernel here sums in.  `wrong` names one deliberate defect (WRONG_KERNELS).
Each returns a dict of outputs.  The key decides the check (hold()):
  'n_*'   counted output (an integer): exact
  'x_*'   fp32 array that must be bit-equal to the reference's
  0-d     scalar:  |got - ref| <= max(R * |cpu - ref|, SCALAR_RTOL * |ref|)
  else    tensor:  e_got <= R * e_cpu + FLOOR,  e_* = relative L2 distance to the float64 reference
R and FLOOR are those of the split-operand tests (split_cases.py); SCALAR_RTOL = 1e-5 is the project's scalar tolerance against
float64 (test_gradient_error_budget_vs_float64).  The first term of the scalar bar keeps the confident-logit regime honest, where
torch's own fp32 BCE is 6e-5 off."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from split_cases import FLOOR, R

SCALAR_RTOL = 1.0e-5
f32, f64 = np.float32, np.float64


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def rel(x, ref):
    """relative L2 distance; an all-zero reference is met only by an all-zero result"""
    x, ref = np.asarray(x, f64), np.asarray(ref, f64)
    d, n = float(np.linalg.norm(x - ref)), float(np.linalg.norm(ref))
    return 0.0 if d == 0.0 else (float('inf') if n == 0.0 else d / n)


CHAIN = 256


def seq_rows(x):
    """fp32 sum of every row of a 2-d array in sequential chains of CHAIN terms (np.cumsum adds in order), the chains' sums added the
    same way.  The longest chain one lane of these kernels adds is 65 terms (the regulariser's 4100 columns over 64 lanes; the KL's
    16384 values over 256 lanes are 64), so this is four times as bad an order as any of them has.  ONE chain over a whole
    reduction is not a summation order a kernel here could have, and no bar near 1e-5 would pass it: over the 2^21 + 7 positive terms
    of the largest image case it is 6e-3 off, over 16384 of them 4e-5."""
    x = np.asarray(x, f32)
    while x.shape[1] > 1:
        pad = -x.shape[1] % CHAIN
        if pad:
            x = np.concatenate([x, np.zeros((x.shape[0], pad), f32)], 1)
        x = np.cumsum(x.reshape(x.shape[0], -1, CHAIN), axis=2, dtype=f32)[:, :, -1]
    return x[:, 0]


def seq_sum(x):
    x = np.asarray(x, f32).reshape(1, -1)
    return f32(seq_rows(x)[0]) if x.size else f32(0)


def hold(case, got, cpu, ref, say=print):
    """the bar on every output of the reference; -> list of (key, figures) that miss it.  Prints each figure first."""
    bad = []
    for k, want in ref.items():
        g = got[k]
        if k.startswith('n_'):
            ok = int(g) == int(want)
            say(f'{case} {k}: got {int(g)}  want {int(want)}')
            if not ok:
                bad.append((k, int(g), int(want)))
        elif k.startswith('x_'):
            g, want = np.ascontiguousarray(g), np.ascontiguousarray(want)
            ok = g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes()
            say(f'{case} {k}: bit-equal {ok}')
            if not ok:
                bad.append((k, 'not bit-equal'))
        elif np.ndim(want) == 0:
            e_got, e_cpu = abs(float(g) - float(want)), abs(float(cpu[k]) - float(want))
            bar = max(R * e_cpu, SCALAR_RTOL * abs(float(want)))
            say(f'{case} {k}: |hip-ref| {e_got:.3e}  |cpu-ref| {e_cpu:.3e}  ref {float(want):.6e}  rel {e_got / abs(float(want)) if want else 0:.2e}  bar {bar:.3e}')
            if not (np.isfinite(float(g)) and e_got <= bar):
                bad.append((k, e_got, e_cpu, bar))
        else:
            finite = bool(np.all(np.isfinite(g)))
            e_got, e_cpu = (rel(g, want) if finite else float('inf')), rel(cpu[k], want)
            ratio = e_got / e_cpu if e_cpu > 0 else float('inf' if e_got > 0 else 0)
            say(f'{case} {k}: e_hip {e_got:.3e}  e_cpu {e_cpu:.3e}  e_hip/e_cpu {ratio:.2f}  bar {R * e_cpu + FLOOR:.3e}')
            if not e_got <= R * e_cpu + FLOOR:
                bad.append((k, e_got, e_cpu))
    return bad


def case_id(case):
    return '-'.join(('x'.join(str(v) for v in c) if isinstance(c, tuple) else f'{c:g}' if isinstance(c, float) else str(c)) for c in case)


# =====================================================================================================================
# latent head:  sigma = exp(log_std), z = mu + eps sigma;  d_mu = g_z, d_log_std = (g_z eps + g_sigma) sigma
# =====================================================================================================================
LATENT_COUNTS = (1, 255, 257, 2048 * 256 + 13)             # one lane, under / over a block, past the 2048-block grid cap
LATENT_CASES = [(n, mode) for n in LATENT_COUNTS for mode in ('both', 'z', 'sigma')]       # which upstream gradients exist


def latent_inputs(case):
    n, mode = case
    rs = _rs('latent', case)
    return dict(n=n, mode=mode, mu=rs.standard_normal(n).astype(f32), ls=rs.uniform(-12.0, 4.0, n).astype(f32),
                eps=rs.standard_normal(n).astype(f32), gz=rs.standard_normal(n).astype(f32), gs=rs.standard_normal(n).astype(f32))


def _latent(inp, dt, exp, fma):
    mu, ls, eps = (inp[k].astype(dt) for k in ('mu', 'ls', 'eps'))
    gz = inp['gz'].astype(dt) if inp['mode'] != 'sigma' else np.zeros(inp['n'], dt)
    gs = inp['gs'].astype(dt) if inp['mode'] != 'z' else np.zeros(inp['n'], dt)
    sigma = exp(ls)
    return dict(sigma=sigma, z=fma(eps, sigma, mu), d_mu=gz, d_ls=(gz * eps + gs) * sigma)


def latent_ref(inp):
    return _latent(inp, f64, np.exp, lambda a, b, c: a * b + c)


def latent_cpu(inp):
    """torch fp32: exp, addcmul"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, f32))
    return _latent(inp, f32, lambda x: t(x).exp().numpy(), lambda a, b, c: torch.addcmul(t(c), t(a), t(b)).numpy())


def latent_chain(inp, wrong=None):
    return _latent(inp, f32, np.exp, lambda a, b, c: (a * b + c).astype(f32))


# =====================================================================================================================
# beta-KL:  beta | mean_b sum_z KL(N(mu, sigma) || N(m0, s0)) - c |
# =====================================================================================================================
KLD_SHAPES = ((1, 1), (3, 700), (256, 32), (1024, 16))     # one element; a ragged second pass of the one-workgroup loop (2100 values);
#                                                            four and eight whole passes
KLD_CASES = [(shape, prior, cap, beta) for shape in KLD_SHAPES for prior in ('std', 'prior') for cap in (0.0, 0.5, 2.0)
             for beta in (4.0, 0.001)]                      # cap: the capacity as a multiple of the KL itself (0: no capacity tensor)
KLD_UPSTREAM = 0.75


def kld_inputs(case):
    (b, z), prior, cap, beta = case
    rs = _rs('kld', case)
    inp = dict(b=b, z=z, beta=beta, mu=rs.standard_normal((b, z)).astype(f32), sigma=np.exp(rs.uniform(-2.0, 1.0, (b, z))).astype(f32),
               pm=None, ps=None, cap=None)
    if prior == 'prior':
        inp['pm'] = rs.standard_normal((b, z)).astype(f32)
        inp['ps'] = rs.uniform(0.3, 3.0, (b, z)).astype(f32)
    if cap:
        inp['cap'] = f32(cap * _kld_value(inp))
    return inp


def _kld_value(inp):
    mu, s = inp['mu'].astype(f64), inp['sigma'].astype(f64)
    m0 = 0.0 if inp['pm'] is None else inp['pm'].astype(f64)
    s0 = 1.0 if inp['ps'] is None else inp['ps'].astype(f64)
    return float((np.log(s0 / s) + (s * s + (mu - m0) ** 2) / (2.0 * s0 * s0) - 0.5).sum() / inp['b'])


def kld_ref(inp):
    mu, s = inp['mu'].astype(f64), inp['sigma'].astype(f64)
    m0 = 0.0 if inp['pm'] is None else inp['pm'].astype(f64)
    s0 = 1.0 if inp['ps'] is None else inp['ps'].astype(f64)
    kl = _kld_value(inp)
    c = 0.0 if inp['cap'] is None else float(inp['cap'])
    k = KLD_UPSTREAM * float(f32(inp['beta'])) * np.sign(kl - c) / inp['b']
    return dict(loss=f64(float(f32(inp['beta'])) * abs(kl - c)), d_mu=k * (mu - m0) / (s0 * s0), d_sigma=k * (s / (s0 * s0) - 1.0 / s))


def kld_cpu(inp):
    """torch.distributions.kl in fp32, gradients by autograd"""
    mu, s = (torch.from_numpy(inp[k]).requires_grad_(True) for k in ('mu', 'sigma'))
    pm = torch.zeros_like(mu) if inp['pm'] is None else torch.from_numpy(inp['pm'])
    ps = torch.ones_like(mu) if inp['ps'] is None else torch.from_numpy(inp['ps'])
    kl = torch.distributions.kl.kl_divergence(torch.distributions.Normal(mu, s), torch.distributions.Normal(pm, ps)).sum(1).mean()
    loss = inp['beta'] * (kl - (0.0 if inp['cap'] is None else float(inp['cap']))).abs()
    (KLD_UPSTREAM * loss).backward()
    return dict(loss=loss.detach().numpy(), d_mu=mu.grad.numpy(), d_sigma=s.grad.numpy())


def kld_chain(inp, wrong=None):
    """kl_elem (vae_finish.h) and kld_bwd_kernel in fp32 numpy, one sequential sum"""
    mu, s = inp['mu'], inp['sigma']
    m0 = f32(0) if inp['pm'] is None else inp['pm']
    s0 = f32(1) if inp['ps'] is None else inp['ps']
    r, d = s / s0, (mu - m0) / s0
    var = r * r
    kl = f32(seq_sum(f32(0.5) * (var + d * d - f32(1) - np.log(var))) * (f32(1) / f32(inp['b'])))
    c = f32(0) if inp['cap'] is None else inp['cap']
    k = f32(f32(KLD_UPSTREAM) * f32(inp['beta']) * np.sign(kl - c) * (f32(1) / f32(inp['b'])))
    q = np.ones_like(mu) if wrong == 'prior sigma ignored in the KL gradient' else s0 * s0
    return dict(loss=f32(f32(inp['beta']) * abs(kl - c)), d_mu=k * (mu - m0) / q, d_sigma=k * (s / q - f32(1) / s))


# =====================================================================================================================
# all-pairs attribute regulariser:  sum_d gamma / NC^2 sum_ij | tanh(delta (z_i - z_j)) - sign(a_i - a_j) |
# =====================================================================================================================
REG_GAMMA = 10.0
REG_UPSTREAM = 3.0
REG_CHUNK = 2048                                            # regloss.h
# name -> (rows, row0, columns, ldz, ldl, dims).  Square forms: rows == columns, row0 = 0.  Row-block forms: `rows` rows
# starting at row0 of a batch of `columns`.
_rs16 = _rs('reg dims 16')
REG_SHAPES = {
    'n1':        (1, 0, 1, 10, 6, (4,)),                        # a single row: every term is the diagonal
    'n7':        (7, 0, 7, 10, 6, (1, 2, 3, 4, 5)),             # under one block of 8 rows
    'n9':        (9, 0, 9, 10, 6, (5, 1, 3, 2, 4)),             # one row over a block; dims unsorted
    'n300r16':   (300, 0, 300, 16, 16, tuple(int(d) for d in _rs16.permutation(16))),    # 4800 row sums: past one 4096 pass of the finish
    'n300ld':    (300, 0, 300, 32, 17, (16, 0, 9)),             # ldz != ldl; 9600 dz entries
    'n2049':     (2049, 0, 2049, 10, 6, (5, 2)),                # one column over REG_CHUNK
    'n4100':     (4100, 0, 4100, 10, 6, (0, 3)),                # three chunks, the last ragged
    'rows5':     (5, 1030, 2051, 10, 6, (1, 4)),                # row blocks against 2051 columns
    'rows121':   (121, 1900, 2051, 10, 6, (3, 2)),
    'repeat200': (200, 0, 200, 10, 6, (2,)),                    # 40 copies each of 5 latent values, the attribute tied to the value
}
REG_CASES = ([(s, delta, attr) for s in ('n1', 'n7', 'n9', 'rows5') for delta in (1.0, 10.0, 50.0) for attr in ('levels', 'cont')] +
             # the larger shapes reach paths of the launch geometry, not of the pair arithmetic: every delta and both attribute kinds
             # once among them, every shape at least twice
             [('n300r16', 1.0, 'levels'), ('n300r16', 10.0, 'cont'), ('n300r16', 50.0, 'levels'),
              ('n300ld', 1.0, 'cont'), ('n300ld', 50.0, 'cont'), ('n2049', 1.0, 'cont'), ('n2049', 50.0, 'levels'),
              ('n4100', 10.0, 'levels'), ('rows121', 10.0, 'cont'), ('rows121', 1.0, 'levels'),
              ('repeat200', 1.0, 'tied'), ('repeat200', 10.0, 'tied'), ('repeat200', 50.0, 'tied')])


def reg_inputs(case):
    shape, delta, attr = case
    rows, row0, cols, ldz, ldl, dims = REG_SHAPES[shape]
    rs = _rs('reg', case)
    z = rs.standard_normal((cols, ldz)).astype(f32)
    if attr == 'levels':
        lab = rs.randint(0, 4, (cols, ldl)).astype(f32)       # many ties
    else:
        lab = rs.random_sample((cols, ldl)).astype(f32)
    if attr == 'tied':                                          # off-diagonal pairs with tanh == 0 and sign == 0: e == 0 where sech^2 == 1
        lvl = rs.permutation(np.repeat(np.arange(5), cols // 5))
        for d in dims:
            z[:, d] = np.array([-1.5, -0.25, 0.0, 0.75, 2.0], f32)[lvl]
            lab[:, d] = lvl.astype(f32)
    return dict(rows=rows, row0=row0, cols=cols, ldz=ldz, ldl=ldl, dims=dims, delta=delta, z=z, lab=lab)


def _reg_scales(inp):
    nn = float(inp['cols']) * float(inp['cols'])
    return f32(REG_GAMMA / nn), f32(2.0 * REG_GAMMA * inp['delta'] / nn)          # arvae_reg_loss's fp32 constants


def _reg_assemble(inp, dt, row_sums, total):
    """loss and dz from per-dimension row sums; row_sums(xr, ar, xc, ac) -> (row_loss, row_grad), total(list of row_loss) -> sum"""
    rows, row0 = inp['rows'], inp['row0']
    z, lab = inp['z'].astype(dt), inp['lab'].astype(dt)
    ls, gs = (dt(v) for v in _reg_scales(inp))
    dz = np.zeros((rows, inp['ldz']), dt)
    rl = []
    for d in inp['dims']:
        l, g = row_sums(z[row0:row0 + rows, d], lab[row0:row0 + rows, d], z[:, d], lab[:, d])
        rl.append(l)
        dz[:, d] = (gs * g) * dt(REG_UPSTREAM)
    keep = np.ones(inp['ldz'], bool)
    keep[list(inp['dims'])] = False
    return dict(loss=dt(total(rl) * ls), dz=dz, x_dz_outside=np.ascontiguousarray(dz[:, keep], f32))


def _row_blocks(n, step=512):
    return [slice(i, min(i + step, n)) for i in range(0, n, step)]


def reg_ref(inp):
    delta = float(f32(inp['delta']))

    def row_sums(xr, ar, xc, ac):
        l, g = np.empty(len(xr)), np.empty(len(xr))
        for b in _row_blocks(len(xr)):                          # (one dimension and 512 rows of the pair matrix at a time)
            t = np.tanh(delta * (xr[b, None] - xc[None, :]))
            s = np.sign(ar[b, None] - ac[None, :])
            l[b] = np.abs(t - s).sum(1)
            g[b] = ((1.0 - t * t) * np.sign(t - s)).sum(1)
        return l, g
    return _reg_assemble(inp, f64, row_sums, lambda rl: float(np.concatenate(rl).sum()))


def _reg_pairs_f32(inp, xr, ar, xc, ac, wrong=None, jitter=None):
    """the kernel's DOCUMENTED formula (regloss.h tanh_sech2) in fp32 numpy: e = exp(-2|x|), r = 1/(1+e), t = +-(1-e) r,
    s2 = 4 e r^2 -> (|t - s|, s2 sgn(t - s)) over the pair matrix.  jitter: a RandomState that moves e and r by -1, 0 or +1 ulp"""
    x = f32(inp['delta']) * (xr[:, None] - xc[None, :])
    e = np.exp(f32(-2) * np.abs(x))
    if jitter is not None:
        e = _ulp_jitter(e, jitter)
    r = f32(1) / (f32(1) + e)
    if jitter is not None:
        r = _ulp_jitter(r, jitter)
    m = (f32(1) - e) * r
    t = np.where(x < 0, -m, m)
    s = np.sign(ar[:, None] - ac[None, :])
    err = t - s
    sg = np.sign(err)
    if wrong == 'sign at e == 0 taken as +1':
        sg = np.where(err == 0, f32(1), sg)
    return np.abs(err), f32(4) * e * r * r * sg


def _ulp_jitter(v, rs):
    k = rs.randint(-1, 2, v.shape).astype(np.int32)
    out = (v.view(np.int32) + k).view(f32)
    return np.where((v > 0) & np.isfinite(out) & (out > 0), out, v)


def reg_cpu(inp, jitter_seed=None):
    """fp32 restatement of the documented formula, row sums in fp32 (numpy's pairwise np.sum)"""
    jitter = None if jitter_seed is None else np.random.RandomState(jitter_seed)

    def row_sums(xr, ar, xc, ac):
        l, g = np.empty(len(xr), f32), np.empty(len(xr), f32)
        for b in _row_blocks(len(xr)):
            pl, pg = _reg_pairs_f32(inp, xr[b], ar[b], xc, ac, jitter=jitter)
            l[b], g[b] = pl.sum(1, dtype=f32), pg.sum(1, dtype=f32)
        return l, g
    return _reg_assemble(inp, f32, row_sums, lambda rl: np.concatenate(rl).sum(dtype=f32))


def reg_chain(inp, wrong=None):
    """the same formula with every sum sequential"""
    def row_sums(xr, ar, xc, ac):
        if wrong == 'columns of the second REG_CHUNK skipped':
            keep = np.ones(len(xc), bool)
            keep[REG_CHUNK:2 * REG_CHUNK] = False
            xc, ac = xc[keep], ac[keep]
        l, g = np.empty(len(xr), f32), np.empty(len(xr), f32)
        for b in _row_blocks(len(xr)):
            pl, pg = _reg_pairs_f32(inp, xr[b], ar[b], xc, ac, wrong=wrong)
            l[b], g[b] = seq_rows(pl), seq_rows(pg)
        return l, g
    out = _reg_assemble(inp, f32, row_sums, lambda rl: seq_sum(np.concatenate(rl)))
    n = inp['cols']
    if wrong == 'diagonal left out of the N^2 mean' and n > 1:
        out['loss'] = f32(out['loss'] * f32(n) / f32(n - 1))
        out['dz'] = out['dz'] * (f32(n) / f32(n - 1))
    if wrong == 'one share of a dimension\'s gradient lost':     # the row share without the (equal) column share
        out['dz'] = out['dz'] * f32(0.5)
    return out


# =====================================================================================================================
# image reconstruction term: sum over all pixels / batch of BCE-with-logits or (sigmoid - x)^2, pixel accuracy, d/dlogits
# =====================================================================================================================
IMAGE_SHAPES = ((1, 1), (1, 3), (3, 1, 5, 7), (4, 1, 64, 64), (2, 4099), (1, (1 << 21) + 7))
#                tail only; tail only (3); 105 = 26 x 4 + 1; no tail, 16 blocks; 8198 = tail of 2; 1024-block cap passed (2 sweeps) + tail of 3
IMAGE_CASES = [(dist, shape, regime, target) for dist in ('bernoulli', 'gaussian') for shape in IMAGE_SHAPES
               for regime in ('mixed', 'confident', 'extreme') for target in ('binary', 'grey')]


def image_inputs(case):
    dist, shape, regime, target = case
    rs = _rs('image', case)
    n = int(np.prod(shape))
    x = (rs.random_sample(n) < 0.3).astype(f32) if target == 'binary' else rs.random_sample(n).astype(f32)
    if target == 'grey':
        x[::11] = 0.5
    if regime == 'mixed':
        l = (3.0 * rs.standard_normal(n)).astype(f32)
        l[::7] = 0.0
        l[3::7] = -0.0
    elif regime == 'confident':                                 # a trained model: the target's sign, 0.2 % wrong
        l = rs.uniform(6.0, 16.0, n) * np.where(x >= 0.5, 1.0, -1.0) * np.where(rs.random_sample(n) < 0.002, -1.0, 1.0)
    else:                                                       # both signs against both targets
        l = rs.choice([30.0, 88.0, 100.0, 1.0e4], n) * rs.choice([-1.0, 1.0], n)
    return dict(dist=dist, shape=shape, batch=shape[0], logits=np.asarray(l, f32).reshape(shape), x=x.reshape(shape))


def _n_correct(l, x):
    return int(np.count_nonzero((l >= 0) == (x >= 0.5)))


def image_ref(inp):
    l, x, b = inp['logits'].astype(f64), inp['x'].astype(f64), inp['batch']
    e = np.exp(-np.abs(l))
    sig = np.where(l >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    if inp['dist'] == 'bernoulli':
        loss, dl = (np.maximum(l, 0.0) - l * x + np.log1p(e)).sum() / b, (sig - x) / b
    else:
        loss, dl = ((sig - x) ** 2).sum() / b, 2.0 * (sig - x) * sig * (1.0 - sig) / b
    return dict(loss=f64(loss), dlogits=dl, n_correct=_n_correct(inp['logits'], inp['x']))


def image_cpu(inp):
    """torch fp32: F.binary_cross_entropy_with_logits(reduction='sum') / batch, or the oracle's Gaussian form; autograd"""
    l, x = torch.from_numpy(inp['logits']).requires_grad_(True), torch.from_numpy(inp['x'])
    if inp['dist'] == 'bernoulli':
        loss = F.binary_cross_entropy_with_logits(l, x, reduction='sum') / inp['batch']
    else:
        loss = ((torch.sigmoid(l) - x) ** 2).sum() / inp['batch']
    loss.backward()
    return dict(loss=loss.detach().numpy(), dlogits=l.grad.numpy(), n_correct=int(((l.detach() >= 0) == (x >= 0.5)).sum()))


def image_chain(inp, wrong=None):
    """the image term in fp32 numpy, sums in chains.  Bernoulli: recon_elem's formula (common.h) with libm's exp / log for the
    hardware's.  Gaussian: the sigmoid as ONE fp32 primitive, as torch has it, then 2 (sig - x) sig (1 - sig) in fp32 (the kernel
    evaluates this term in float64).  An fp32 e * rcp(1 + e) in its place is four roundings deep before the gradient squares it: on
    the single element of (gaussian, (1, 1), confident, binary) that is 3.7e-7 off, above a bar of 2.9e-7 that torch sets by landing
    within 0.8 ulp there -- what recon_elem gave, bit for bit, before it changed."""
    l, x = inp['logits'].ravel(), inp['x'].ravel()
    inv_b = f32(1) / f32(inp['batch'])
    live = np.ones(l.size, bool)
    if wrong == 'count & 3 tail dropped':
        live[l.size & ~3:] = False
    e = np.exp(-np.abs(l))
    u = f32(1) + e
    r = f32(1) / u
    sig = np.where(l >= 0, r, e * r) if inp['dist'] == 'bernoulli' else torch.sigmoid(torch.from_numpy(l)).numpy()
    if inp['dist'] == 'bernoulli':
        log1p = np.log(u) if wrong == 'log(1 + e) without the correction term' else np.log(u) - ((u - f32(1)) - e) * r
        term, dl = np.maximum(l, f32(0)) - l * x + log1p, (sig - x) * inv_b
    else:
        df = sig - x
        term, dl = df * df, f32(2) * df * sig * (f32(1) - sig) * inv_b
    return dict(loss=f32(seq_sum(term[live]) * inv_b), dlogits=np.where(live, dl, f32(0)).reshape(inp['shape']),
                n_correct=_n_correct(l[live], x[live]))


# =====================================================================================================================
# token reconstruction term: mean cross entropy over rows, top-1 count (first maximum on ties), d/dweights
# =====================================================================================================================
TOKEN_SHAPES = ((1, 1), (1, 2), (63, 35), (64, 35), (65, 48), (65, 49), (200, 130), (65536 + 70, 5), (65536 + 70, 49))
#   one column; fewer columns than lanes per row; one row under / exactly / one over a 64-row pass; the widest staged vocabulary and the
#   first unstaged one; a real note vocabulary (unstaged, several passes); rows past one sweep of the 1024-block grid, staged and not
TOKEN_CASES = [(shape, kind) for shape in TOKEN_SHAPES for kind in ('normal', 'wide', 'relu')]


def token_inputs(case):
    (rows, v), kind = case
    rs = _rs('token', case)
    w = rs.standard_normal((rows, v))
    tgt = rs.randint(0, v, rows).astype(np.int64)
    if kind == 'wide':
        w = 30.0 * w
    if kind == 'relu':                                          # the decoder's logits: ReLU outputs, mostly zeros
        w = np.maximum(w - 1.0, 0.0)
        w[::5] = 0.0                                            # all-zero rows: the first maximum is column 0
        tgt[::10] = 0
        # tied maxima whose positions fall in different j % 4 classes (the kernel's four lanes per row; in (3, 4) the lower index
        # is in the higher class), the target on the first of them in one round of the pairs and on the second in the next
        pairs = [(a, b) for a, b in ((3, 4), (1, 6), (2, v - 1), (0, v - 1), (v - 2, v - 1)) if 0 <= a < b < v and a % 4 != b % 4]
        for i, r in enumerate(range(2, rows, 5)):
            if pairs:
                a, b = pairs[i % len(pairs)]
                w[r, a] = w[r, b] = w[r].max() + 1.5
                tgt[r] = a if (i // len(pairs)) % 2 == 0 else b
    tgt[0], tgt[-1] = 0, v - 1
    return dict(rows=rows, v=v, w=np.asarray(w, f32), tgt=tgt)


def _n_top1(w, tgt):
    return int(np.count_nonzero(np.argmax(w, 1) == tgt))        # np.argmax: the first maximum


def token_ref(inp):
    w, tgt, rows = inp['w'].astype(f64), inp['tgt'], inp['rows']
    mx = w.max(1, keepdims=True)
    p = np.exp(w - mx)
    se = p.sum(1, keepdims=True)
    loss = (mx[:, 0] + np.log(se[:, 0]) - w[np.arange(rows), tgt]).sum() / rows
    dw = p / se
    dw[np.arange(rows), tgt] -= 1.0
    return dict(loss=f64(loss), dw=dw / rows, n_correct=_n_top1(inp['w'], tgt))


def token_cpu(inp):
    """torch fp32: F.cross_entropy (mean), autograd, argmax"""
    w, tgt = torch.from_numpy(inp['w']).requires_grad_(True), torch.from_numpy(inp['tgt'])
    loss = F.cross_entropy(w, tgt)
    loss.backward()
    return dict(loss=loss.detach().numpy(), dw=w.grad.numpy(), n_correct=int((w.detach().argmax(1) == tgt).sum()))


def token_chain(inp, wrong=None):
    """token_recon_body in fp32 numpy: first maximum, sequential sums"""
    w, tgt, rows, v = inp['w'], inp['tgt'], inp['rows'], inp['v']
    idx = np.arange(rows)
    if wrong == 'last maximum on ties':
        arg = v - 1 - np.argmax(w[:, ::-1], 1)
    elif wrong == 'maximum over one lane\'s quarter of the row':
        arg = 4 * np.argmax(w[:, ::4], 1)
    else:
        arg = np.argmax(w, 1)
    mx = w[idx, arg]
    with np.errstate(over='ignore', invalid='ignore'):
        p = np.exp(w - mx[:, None])
        se = seq_rows(p)
        inv_rows = f32(1) / f32(rows)
        loss = f32(seq_sum(mx + np.log(se) - w[idx, tgt]) * inv_rows)
        dw = p * (f32(1) / se)[:, None]
        dw[idx, tgt] -= f32(1)
    return dict(loss=loss, dw=dw * inv_rows, n_correct=int(np.count_nonzero(arg == tgt)))


# =====================================================================================================================
# Adam: ONE update from a given fp32 state.  The bar is on p_new - p_old, m and v.
# =====================================================================================================================
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1.0e-3, 0.9, 0.999, 1.0e-8
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_SCALES = (1.0, 0.125, 1.0 / 3.0)
ADAM_STATUS = ('none', 'clear', 'failed')                   # no status words; all zero; status[0] = 1: the update is skipped
# (count, step, grad_scale, zero_grad, status): the small counts with every (step, grad_scale), zero_grad and the status cycling so
# that all six combinations come twice per count; the count past the grid cap (2048 blocks x 256 lanes x 4) four times
ADAM_CASES = [(n, step, gs, bool(i % 2), ADAM_STATUS[i % 3]) for n in (1, 3, 4, 10007)
              for i, (step, gs) in enumerate((s, g) for s in ADAM_STEPS for g in ADAM_SCALES)] + \
             [((1 << 21) + 5, 1, 1.0, True, 'none'), ((1 << 21) + 5, 2, 0.125, False, 'clear'),
              ((1 << 21) + 5, 1000, 1.0 / 3.0, True, 'failed'), ((1 << 21) + 5, 100000, 1.0, False, 'failed')]
ADAM_STATUS4 = 7                                            # skipped updates counted so far


def adam_inputs(case):
    n, step, gs, zero_grad, status = case
    rs = _rs('adam', case)
    mag = 10.0 ** rs.uniform(-8.0, 3.0, n)                      # log-uniform gradient magnitudes
    g = (mag * rs.choice([-1.0, 1.0], n)).astype(f32)
    zero = rs.random_sample(n) < 0.1
    if n >= 4:
        zero[1] = True
    g[zero] = 0.0                                               # exact-zero gradients ...
    if step == 1:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    else:
        m = (mag * gs * rs.uniform(-1.0, 1.0, n)).astype(f32)
        v = ((mag * gs) ** 2 * rs.uniform(0.2, 2.0, n)).astype(f32)
        m[zero], v[zero] = 0.0, 0.0                             # ... on zero moments: 0 / (0 + eps)
    st = None if status == 'none' else np.array([1 if status == 'failed' else 0, 0, 0, 0, ADAM_STATUS4, 0, 0, 0], np.int32)
    return dict(n=n, step=step, gs=f32(gs), zero_grad=zero_grad, status=st, p=rs.standard_normal(n).astype(f32), g=g, m=m, v=v)


def adam_constants(step, dt=f64, bias_step=None):
    """arvae_adam_step's fp32 launch constants"""
    bs = step if bias_step is None else bias_step
    bc1, bc2 = 1.0 - ADAM_B1 ** bs, 1.0 - ADAM_B2 ** bs
    c = dict(step_size=f32(ADAM_LR / bc1), inv_bc2_sqrt=f32(1.0 / np.sqrt(bc2)), b1=f32(ADAM_B1), b2=f32(ADAM_B2),
             omb1=f32(1.0 - ADAM_B1), omb2=f32(1.0 - ADAM_B2), eps=f32(ADAM_EPS))
    return {k: dt(v) for k, v in c.items()}


def _adam_exact(inp):
    """what is exact whatever the arithmetic: the cleared or untouched gradient, the status counter, a skipped update"""
    failed = inp['status'] is not None and inp['status'][0] != 0
    out = dict(x_g=np.zeros(inp['n'], f32) if inp['zero_grad'] else inp['g'].copy())
    if inp['status'] is not None:
        out['n_status4'] = ADAM_STATUS4 + (1 if failed else 0)
    if failed:
        out.update(x_p=inp['p'].copy(), x_m=inp['m'].copy(), x_v=inp['v'].copy())
    return out, failed


def _adam(inp, dt, c, gscale_v=True):
    out, failed = _adam_exact(inp)
    if failed:
        return out
    p, g0, m, v = (inp[k].astype(dt) for k in ('p', 'g', 'm', 'v'))
    g = g0 * dt(inp['gs'])
    gv = g if gscale_v else g0
    m = c['b1'] * m + c['omb1'] * g
    v = c['b2'] * v + c['omb2'] * gv * gv
    upd = c['step_size'] * (m / (np.sqrt(v) * c['inv_bc2_sqrt'] + c['eps']))
    # fp32: the difference of the stored p to p_old (exact in float64), as the GPU test forms it
    out.update(dp=(p - upd).astype(f64) - p.astype(f64) if dt is f32 else -upd, m=m, v=v)
    return out


def adam_ref(inp):
    return _adam(inp, f64, adam_constants(inp['step']))


def adam_cpu(inp):
    """oracle.losses.adam_step on the scaled gradient"""
    from oracle import losses
    out, failed = _adam_exact(inp)
    if failed:
        return out
    p, m, v = losses.adam_step(inp['p'], inp['g'] * inp['gs'], inp['m'], inp['v'], inp['step'], ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS)
    out.update(dp=p.astype(f64) - inp['p'].astype(f64), m=m, v=v)
    return out


def adam_chain(inp, wrong=None):
    """adam_kernel in fp32 numpy"""
    bias_step = max(inp['step'] - 1, 1) if wrong == 'bias correction of step - 1' else None
    return _adam(inp, f32, adam_constants(inp['step'], f32, bias_step), gscale_v=wrong != 'grad_scale applied to m but not to v')


# =====================================================================================================================
# scale_by_scalar: y = g[0] x, bit-equal to the fp32 product
# =====================================================================================================================
SCALE_CASES = [(1,), (1023,), ((1 << 20) + 1,)]             # one lane; four blocks, the last ragged; 1025 blocks, one lane in the last


def scale_inputs(case):
    (n,) = case
    rs = _rs('scale', case)
    return dict(n=n, g=f32(rs.standard_normal() * 3.0), x=(rs.standard_normal(n) * np.exp(3.0 * rs.standard_normal(n))).astype(f32))


def scale_ref(inp):
    return dict(x_y=(inp['g'] * inp['x']).astype(f32))


# =====================================================================================================================
# deliberate defects the bar must catch: name -> (family, chain function).  test_loss_cases.py finds a case each one fails.
# =====================================================================================================================
FAMILIES = {
    'latent': (LATENT_CASES, latent_inputs, latent_ref, latent_cpu, latent_chain),
    'kld': (KLD_CASES, kld_inputs, kld_ref, kld_cpu, kld_chain),
    'reg': (REG_CASES, reg_inputs, reg_ref, reg_cpu, reg_chain),
    'image': (IMAGE_CASES, image_inputs, image_ref, image_cpu, image_chain),
    'token': (TOKEN_CASES, token_inputs, token_ref, token_cpu, token_chain),
    'adam': (ADAM_CASES, adam_inputs, adam_ref, adam_cpu, adam_chain),
}
# name -> (family, a case of the table it must fail)
WRONG_KERNELS = {
    'count & 3 tail dropped': ('image', ('bernoulli', (1, 3), 'mixed', 'binary')),
    # (one confident pixel: from 105 pixels on the few flipped ones and the 1e-5 term of the scalar bar cover what this loses)
    'log(1 + e) without the correction term': ('image', ('bernoulli', (1, 1), 'confident', 'binary')),
    'last maximum on ties': ('token', ((63, 35), 'relu')),
    'maximum over one lane\'s quarter of the row': ('token', ((65, 49), 'normal')),
    'diagonal left out of the N^2 mean': ('reg', ('n7', 1.0, 'cont')),
    'sign at e == 0 taken as +1': ('reg', ('repeat200', 10.0, 'tied')),
    'one share of a dimension\'s gradient lost': ('reg', ('n9', 10.0, 'cont')),
    'prior sigma ignored in the KL gradient': ('kld', ((3, 700), 'prior', 0.5, 4.0)),
    'grad_scale applied to m but not to v': ('adam', (10007, 2, 0.125, False, 'clear')),
    'bias correction of step - 1': ('adam', (10007, 2, 1.0, True, 'none')),
    'columns of the second REG_CHUNK skipped': ('reg', ('n2049', 1.0, 'cont')),
}

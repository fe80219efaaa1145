"""The loss-side kernels (ar-vae_amd/csrc/losses.hip, regloss.h, recon_elem in common.h) against float64, one family at a time through
the public wrappers of ops.py: latent_head, kld_loss, reg_loss, image_recon, token_recon, adam_step, scale_by_scalar.  Every
reference is a closed form on inputs the table chooses, so no activation can flip sides.  Needs a real MI355X.

The tables, the references, the fp32 CPU yardsticks and the bar are in loss_cases.py; test_loss_cases.py proves on the CPU that the
references are right and that the bar passes a correct fp32 kernel and fails the listed wrong ones.  Each case prints e_hip, e_cpu,
their ratio and the bar (scalars: the two absolute errors and the bar).

Case -> path of the kernel it is the smallest shape for: the comments of the tables in loss_cases.py.

No case feeds NaN, infinity or an out-of-range target.

Measured on the MI355X: all 251 cases hold (figures per family: DESIGN.md section 4, item 58).  The first run of this file found
five one- and three-pixel cases of the image term above the bar, and recon_elem (common.h) changed for them:
  bernoulli-1x1-extreme-binary: the loss of l = 88 against x = 1 is log1p(exp(-88)) = 6.05e-39, a denormal; the hardware exp2
      flushed it and the kernel returned 0.  The exponent is now raised by 64 beyond |l| = 80 and the result scaled back: 1.1e-44 off
      (1.8e-6 relative, the rounded product |l| log2(e)), bar 6.1e-44.
  gaussian-1x1-extreme-binary, gaussian-1x3-extreme-binary (l = -30; e |l| x 6e-8 relative off, squared by the gradient: 2.48e-6
      against a bar of 5.11e-7) and gaussian-1x1-confident-binary, gaussian-1x3-confident-binary (l = -7.28: the correctly rounded
      fp32 evaluation of the old formula, the same bits as numpy's, four roundings and a square deep: 3.73e-7 and 5.10e-7 against
      bars of 2.94e-7 and 3.19e-7 that torch set within 0.8 ulp): the Gaussian term is now evaluated in float64 and rounded once,
      1.2e-8 .. 2.9e-8 on these four, e_hip / e_cpu <= 0.76 on every Gaussian case."""
import ctypes

import numpy as np
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _t(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _hold(case, got, cpu, ref):
    bad = lc.hold(lc.case_id(case), got, cpu, ref)
    assert not bad, (lc.case_id(case), bad)


@pytest.mark.parametrize('case', lc.LATENT_CASES, ids=lc.case_id)
def test_latent_head_vs_float64(dev, case):
    """latent_fwd_kernel / latent_bwd_kernel.  The upstream gradients come through autograd (an unused output arrives as zeros);
    with only z or only sigma used the backward kernel is also launched with the other pointer NULL, as the per-layer trainer
    does when a term is switched off: both must hold."""
    from arvae_amd import _lib, ops
    inp = lc.latent_inputs(case)
    mu, ls = _t(inp['mu'], dev, True), _t(inp['ls'], dev, True)
    eps, gz, gs = _t(inp['eps'], dev), _t(inp['gz'], dev), _t(inp['gs'], dev)
    sigma, z = ops.latent_head(mu, ls, eps)
    outs, grads = {'both': ([sigma, z], [gs, gz]), 'z': ([z], [gz]), 'sigma': ([sigma], [gs])}[inp['mode']]
    d_mu, d_ls = torch.autograd.grad(outs, [mu, ls], grads)
    got = dict(sigma=_np(sigma), z=_np(z), d_mu=_np(d_mu), d_ls=_np(d_ls))
    ref, cpu = lc.latent_ref(inp), lc.latent_cpu(inp)
    _hold(case, got, cpu, ref)
    if inp['mode'] != 'both':
        a_mu, a_ls = torch.empty_like(sigma), torch.empty_like(sigma)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().arvae_latent_bwd(p(gz) if inp['mode'] == 'z' else None, p(gs) if inp['mode'] == 'sigma' else None, p(eps),
                                          p(sigma.detach()), inp['n'], p(a_mu), p(a_ls), None)
        assert rc == 0
        torch.cuda.synchronize()
        _hold(case + ('null',), dict(d_mu=_np(a_mu), d_ls=_np(a_ls)), cpu, {k: ref[k] for k in ('d_mu', 'd_ls')})


@pytest.mark.parametrize('case', lc.KLD_CASES, ids=lc.case_id)
def test_kld_vs_float64(dev, case):
    """kld_fwd_kernel / kld_bwd_kernel: N(0, 1) and a general prior, the capacity below and above the KL"""
    from arvae_amd import ops
    inp = lc.kld_inputs(case)
    mu, sigma = _t(inp['mu'], dev, True), _t(inp['sigma'], dev, True)
    pm = None if inp['pm'] is None else _t(inp['pm'], dev)
    ps = None if inp['ps'] is None else _t(inp['ps'], dev)
    cap = None if inp['cap'] is None else _t(np.array([inp['cap']], np.float32), dev)
    loss = ops.kld_loss(mu, sigma, inp['beta'], cap, pm, ps)
    (lc.KLD_UPSTREAM * loss.sum()).backward()
    got = dict(loss=_np(loss).reshape(()), d_mu=_np(mu.grad), d_sigma=_np(sigma.grad))
    _hold(case, got, lc.kld_cpu(inp), lc.kld_ref(inp))


@pytest.mark.parametrize('case', lc.REG_CASES, ids=lc.case_id)
def test_reg_loss_vs_float64(dev, case):
    """reg_loss_kernel + reg_finish_kernel (+ scale_by_scalar for the upstream gradient of 3), square and row-block forms"""
    from arvae_amd import ops
    inp = lc.reg_inputs(case)
    rows, row0 = inp['rows'], inp['row0']
    z_all, lab_all = _t(inp['z'], dev), _t(inp['lab'], dev)
    z = z_all[row0:row0 + rows].clone().requires_grad_(True)
    square = rows == inp['cols']
    loss = ops.reg_loss(z, lab_all[row0:row0 + rows].clone(), inp['dims'], lc.REG_GAMMA, inp['delta'],
                        None if square else z_all, None if square else lab_all)
    (lc.REG_UPSTREAM * loss).backward()
    dz = _np(z.grad)
    keep = np.ones(inp['ldz'], bool)
    keep[list(inp['dims'])] = False
    got = dict(loss=_np(loss), dz=dz, x_dz_outside=np.ascontiguousarray(dz[:, keep]))
    _hold(case, got, lc.reg_cpu(inp), lc.reg_ref(inp))


@pytest.mark.parametrize('case', lc.IMAGE_CASES, ids=lc.case_id)
def test_image_recon_vs_float64(dev, case):
    """image_recon_kernel<DIST> + pair_finish_kernel: the loss, the whole of dlogits, the count of correct pixels"""
    from arvae_amd import ops
    inp = lc.image_inputs(case)
    logits, x = _t(inp['logits'], dev, True), _t(inp['x'], dev)
    loss, acc = ops.image_recon(logits, x, inp['dist'])
    loss.backward()
    got = dict(loss=_np(loss), dlogits=_np(logits.grad), n_correct=round(float(acc) * logits.numel()))
    _hold(case, got, lc.image_cpu(inp), lc.image_ref(inp))


@pytest.mark.parametrize('case', lc.TOKEN_CASES, ids=lc.case_id)
def test_token_recon_vs_float64(dev, case):
    """token_recon_kernel (staged up to 48 columns, straight from memory above) + pair_finish_kernel"""
    from arvae_amd import ops
    inp = lc.token_inputs(case)
    w, tgt = _t(inp['w'], dev, True), _t(inp['tgt'], dev)
    loss, acc = ops.token_recon(w, tgt)
    loss.backward()
    got = dict(loss=_np(loss), dw=_np(w.grad), n_correct=round(float(acc) * inp['rows']))
    _hold(case, got, lc.token_cpu(inp), lc.token_ref(inp))


@pytest.mark.parametrize('case', lc.ADAM_CASES, ids=lc.case_id)
def test_adam_vs_float64(dev, case):
    """adam_kernel<ZERO_G>: one update from a given state; the bar on p_new - p_old, m and v; the gradient arena, the status
    counter and a skipped update bit for bit"""
    from arvae_amd import ops
    inp = lc.adam_inputs(case)
    p, g, m, v = (_t(inp[k], dev) for k in ('p', 'g', 'm', 'v'))
    status = None if inp['status'] is None else _t(inp['status'], dev)
    ops.adam_step(p, g, m, v, inp['step'], lc.ADAM_LR, lc.ADAM_B1, lc.ADAM_B2, lc.ADAM_EPS, grad_scale=float(inp['gs']),
                  zero_grad=inp['zero_grad'], status=status)
    got = dict(dp=_np(p).astype(np.float64) - inp['p'].astype(np.float64), m=_np(m), v=_np(v), x_g=_np(g), x_p=_np(p), x_m=_np(m), x_v=_np(v))
    if status is not None:
        st = _np(status)
        got['n_status4'] = int(st[4])
        assert st[0] == inp['status'][0] and not st[1:4].any() and not st[5:].any()
    _hold(case, got, lc.adam_cpu(inp), lc.adam_ref(inp))


@pytest.mark.parametrize('case', lc.SCALE_CASES, ids=lc.case_id)
def test_scale_by_scalar_is_the_fp32_product(dev, case):
    from arvae_amd import ops
    inp = lc.scale_inputs(case)
    y = ops.scale_by_scalar(_t(np.array(inp['g'], np.float32), dev), _t(inp['x'], dev))
    _hold(case, dict(x_y=_np(y)), {}, lc.scale_ref(inp))

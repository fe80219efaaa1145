"""CPU proof for the float64 tests of the loss-side kernels (loss_cases.py, test_loss_kernels_float64.py):

  1. the float64 references reproduce oracle/losses.py and the committed goldens where the cases overlap: a wrong reference must
     not pass quietly;
  2. for every family and every case the fp32 yardstick itself and a plain fp32 restatement with chained sums pass the bar;
  3. the bar discriminates: every wrong kernel of loss_cases.WRONG_KERNELS fails it on the case named there;
  4. a dimension listed twice is refused by arvae_reg_loss, by the image executor's finishing step and by ops.reg_loss before
     anything is launched (the loss would count it twice, dz has one entry for it).

Runs anywhere (no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_cases as lc
from oracle import losses

torch.set_num_threads(1)


def close(a, b, rtol, atol=0.0):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def G(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ---------------------------------------------------------------------------------------------------------------- 1. references
# (the references take the kernels' fp32 launch constants -- gamma / N^2, beta, 1 / batch -- where the oracle has the float64
# ones: 6e-8 relative apiece, hence rtol 1e-6 and not 1e-12)
@pytest.mark.parametrize('case', [c for c in lc.REG_CASES if c[0] in ('n1', 'n7', 'n9', 'rows5', 'n300ld', 'repeat200')], ids=lc.case_id)
def test_reg_reference_is_the_oracles_closed_form(case):
    inp = lc.reg_inputs(case)
    ref = lc.reg_ref(inp)
    z, lab = inp['z'].astype(np.float64), inp['lab'].astype(np.float64)
    rows = slice(inp['row0'], inp['row0'] + inp['rows'])
    total, dz = 0.0, np.zeros((inp['rows'], inp['ldz']))
    for d in inp['dims']:
        loss, grad = losses.reg_loss_closed_form(z[rows, d], lab[rows, d], lc.REG_GAMMA, inp['delta'], cols_x=z[:, d], cols_a=lab[:, d])
        total += loss
        dz[:, d] = lc.REG_UPSTREAM * grad
    close(ref['loss'], total, rtol=1e-6)
    close(ref['dz'], dz, rtol=1e-6, atol=1e-7 * np.abs(dz).max())


@pytest.mark.parametrize('n', [7, 64, 512])
def test_reg_reference_against_the_golden(golden_dir, n):
    g = G(golden_dir, 'reg_loss.npz')
    x = g[f'n{n}/x']
    for tag in ('cont', 'ties'):
        a = g[f'n{n}/a_{tag}']
        for delta in (1.0, 10.0):
            inp = dict(rows=n, row0=0, cols=n, ldz=2, ldl=2, dims=(1,), delta=delta, z=np.stack([x * 0, x], 1).astype(np.float32),
                       lab=np.stack([a * 0, a], 1).astype(np.float32))
            ref = lc.reg_ref(inp)
            key = f'n{n}_{tag}_d{delta:g}_g{lc.REG_GAMMA:g}'
            close(ref['loss'], g[f'{key}/loss'], rtol=2e-6)                     # (the tolerances of test_oracle_golden.py: fp32 goldens)
            close(ref['dz'][:, 1] / lc.REG_UPSTREAM, g[f'{key}/grad'], rtol=1e-4, atol=2e-7 * lc.REG_GAMMA * delta)
            assert not ref['dz'][:, 0].any()


@pytest.mark.parametrize('case', [c for c in lc.KLD_CASES if c[1] == 'std'], ids=lc.case_id)
def test_kld_reference_is_the_oracles_closed_form(case):
    inp = lc.kld_inputs(case)
    ref = lc.kld_ref(inp)
    sigma = inp['sigma'].astype(np.float64)
    c = 0.0 if inp['cap'] is None else float(inp['cap'])
    val, dmu, dls = losses.kld_closed_form(inp['mu'], np.log(sigma), inp['beta'], c)
    close(ref['loss'], val, rtol=1e-6)
    close(ref['d_mu'], lc.KLD_UPSTREAM * dmu, rtol=1e-6)
    close(ref['d_sigma'] * sigma, lc.KLD_UPSTREAM * dls, rtol=1e-6, atol=1e-12)        # d/d log_std = sigma d/d sigma


@pytest.mark.parametrize('case', [c for c in lc.KLD_CASES if c[1] == 'prior' and c[0] != (1024, 16)], ids=lc.case_id)
def test_kld_reference_with_a_prior_is_torchs_kl_in_float64(case):
    inp = lc.kld_inputs(case)
    ref = lc.kld_ref(inp)
    mu, s = (torch.from_numpy(inp[k]).double().requires_grad_(True) for k in ('mu', 'sigma'))
    q = torch.distributions.Normal(torch.from_numpy(inp['pm']).double(), torch.from_numpy(inp['ps']).double())
    kl = torch.distributions.kl.kl_divergence(torch.distributions.Normal(mu, s), q).sum(1).mean()
    loss = float(np.float32(inp['beta'])) * (kl - (0.0 if inp['cap'] is None else float(inp['cap']))).abs()
    (lc.KLD_UPSTREAM * loss).backward()
    close(ref['loss'], loss.item(), rtol=1e-12)
    close(ref['d_mu'], mu.grad.numpy(), rtol=1e-10, atol=1e-18)
    close(ref['d_sigma'], s.grad.numpy(), rtol=1e-10, atol=1e-18)


@pytest.mark.parametrize('b,z', [(8, 10), (64, 10), (32, 32)])
def test_latent_and_kld_references_against_the_golden(golden_dir, b, z):
    g = G(golden_dir, 'latent_head.npz')
    mu, ls, eps = (g[f'b{b}_z{z}/{k}'].astype(np.float32) for k in ('mu', 'log_std', 'eps'))
    inp = dict(n=mu.size, mode='both', mu=mu.ravel(), ls=ls.ravel(), eps=eps.ravel(), gz=np.ones(mu.size, np.float32), gs=np.zeros(mu.size, np.float32))
    ref = lc.latent_ref(inp)
    close(ref['z'].reshape(b, z), g[f'b{b}_z{z}/z'], rtol=1e-6, atol=1e-6)
    close(ref['d_ls'], (eps.astype(np.float64) * np.exp(ls.astype(np.float64))).ravel(), rtol=1e-12)
    sigma = np.exp(ls.astype(np.float64)).astype(np.float32)
    for c in (0.0, 25.0):
        for beta in (4.0, 0.001):
            kin = dict(b=b, z=z, beta=beta, mu=mu, sigma=sigma, pm=None, ps=None, cap=np.float32(c) if c else None)
            close(lc.kld_ref(kin)['loss'], g[f'b{b}_z{z}_c{c:g}_beta{beta:g}/kld'], rtol=1e-5)


@pytest.mark.parametrize('case', [c for c in lc.IMAGE_CASES if int(np.prod(c[1])) < 100000], ids=lc.case_id)
def test_image_reference_is_the_oracles_terms_in_float64(case):
    inp = lc.image_inputs(case)
    ref = lc.image_ref(inp)
    l, x = torch.from_numpy(inp['logits']).double().requires_grad_(True), torch.from_numpy(inp['x']).double()
    loss = (losses.bce_with_logits_per_batch if inp['dist'] == 'bernoulli' else losses.gaussian_recon_per_batch)(l, x)
    loss.backward()
    close(ref['loss'], loss.item(), rtol=1e-12)
    assert lc.rel(ref['dlogits'], l.grad.numpy()) < 1e-12
    want = float(losses.pixel_accuracy(torch.from_numpy(inp['logits']), torch.from_numpy(inp['x']))) * l.numel()
    assert ref['n_correct'] == round(want)


@pytest.mark.parametrize('b,hw', [(4, 64), (16, 28)])
def test_image_reference_against_the_golden(golden_dir, b, hw):
    g = G(golden_dir, 'recon.npz')
    rs = np.random.RandomState(b * hw)                                           # the golden's inputs (test_oracle_golden.py)
    logits = (3.0 * rs.standard_normal((b, 1, hw, hw))).astype(np.float32)
    logits.ravel()[::97] = 0.0
    x = (rs.random_sample((b, 1, hw, hw)) < 0.2).astype(np.float32)
    if hw == 28:
        x = (x * rs.random_sample(x.shape)).astype(np.float32)
    for dist in ('bernoulli', 'gaussian'):
        ref = lc.image_ref(dict(dist=dist, shape=logits.shape, batch=b, logits=logits, x=x))
        close(ref['loss'], g[f'b{b}_{hw}_{dist}/loss'], rtol=1e-5)
        close(ref['dlogits'].ravel()[::131], g[f'b{b}_{hw}_{dist}/dlogits_samp'], rtol=1e-4, atol=1e-7)
        close(np.abs(ref['dlogits']).sum(), g[f'b{b}_{hw}_{dist}/dlogits_abs_sum'], rtol=1e-5)
        close(ref['n_correct'] / logits.size, g[f'b{b}_{hw}/acc'], rtol=1e-6)


@pytest.mark.parametrize('case', [c for c in lc.TOKEN_CASES if c[0][0] < 1000], ids=lc.case_id)
def test_token_reference_is_the_oracles_cross_entropy_in_float64(case):
    inp = lc.token_inputs(case)
    ref = lc.token_ref(inp)
    w, tgt = torch.from_numpy(inp['w']).double().requires_grad_(True), torch.from_numpy(inp['tgt'])
    loss = losses.cross_entropy_mean(w, tgt)
    loss.backward()
    close(ref['loss'], loss.item(), rtol=1e-12, atol=1e-15)
    close(ref['dw'], w.grad.numpy(), rtol=1e-9, atol=1e-15)
    assert ref['n_correct'] == round(float(losses.top1_accuracy(torch.from_numpy(inp['w']), tgt)) * inp['rows'])
    if case[1] == 'relu' and inp['v'] > 1 and inp['rows'] > 2:                   # the planted ties are there and decide the count
        tied = (inp['w'] == inp['w'].max(1, keepdims=True)).sum(1) > 1
        assert tied.any() and (inp['w'].max(1) == 0).any()
        assert lc.token_chain(inp, 'last maximum on ties')['n_correct'] != ref['n_correct']


@pytest.mark.parametrize('b', [5, 32])
def test_token_reference_against_the_golden(golden_dir, b):
    g = G(golden_dir, 'recon.npz')
    w, tgt = g[f'ce_b{b}/w'], g[f'ce_b{b}/tgt']
    v = w.shape[-1]
    ref = lc.token_ref(dict(rows=w.size // v, v=v, w=w.reshape(-1, v).astype(np.float32), tgt=tgt.reshape(-1)))
    close(ref['loss'], g[f'ce_b{b}/loss'], rtol=1e-5)
    close(ref['n_correct'] / (w.size // v), g[f'ce_b{b}/acc'], rtol=1e-6)
    close(ref['dw'].ravel()[::37], g[f'ce_b{b}/dw_samp'], rtol=1e-4, atol=1e-8)


def test_adam_reference_is_torchs_adam_in_float64():
    """one update of torch.optim.Adam on float64 copies of a case's state (grad_scale 1, step through the optimiser's own
    counter): the reference's formula, order of eps and bias corrections included; the fp32 launch constants are 6e-8 apiece"""
    for case in [c for c in lc.ADAM_CASES if c[0] == 10007 and c[2] == 1.0 and c[4] != 'failed']:
        inp = lc.adam_inputs(case)
        ref = lc.adam_ref(inp)
        p = torch.from_numpy(inp['p']).double().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lc.ADAM_LR, betas=(lc.ADAM_B1, lc.ADAM_B2), eps=lc.ADAM_EPS)
        p.grad = torch.from_numpy(inp['g']).double()
        opt.state[p] = dict(step=torch.tensor(float(inp['step'] - 1)), exp_avg=torch.from_numpy(inp['m']).double(),
                            exp_avg_sq=torch.from_numpy(inp['v']).double())
        opt.step()
        assert lc.rel(ref['dp'], p.detach().numpy() - inp['p'].astype(np.float64)) < 1e-6
        assert lc.rel(ref['m'], opt.state[p]['exp_avg'].numpy()) < 1e-6 and lc.rel(ref['v'], opt.state[p]['exp_avg_sq'].numpy()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2. the bar passes
@pytest.mark.parametrize('family', list(lc.FAMILIES))
def test_yardstick_and_fp32_restatement_pass_the_bar_on_every_case(family):
    cases, inputs, ref_fn, cpu_fn, chain_fn = lc.FAMILIES[family]
    bad = []
    for case in cases:
        inp = inputs(case)
        ref, cpu = ref_fn(inp), cpu_fn(inp)
        assert set(cpu) >= set(ref), case
        bad += [(lc.case_id(case), 'yardstick', b) for b in lc.hold(lc.case_id(case) + ' [yardstick]', cpu, cpu, ref)]
        bad += [(lc.case_id(case), 'restatement', b) for b in lc.hold(lc.case_id(case) + ' [restatement]', chain_fn(inp), cpu, ref)]
    assert not bad, bad


def test_scale_reference_is_the_fp32_product():
    for case in lc.SCALE_CASES:
        inp = lc.scale_inputs(case)
        y = lc.scale_ref(inp)['x_y']
        assert y.dtype == np.float32 and y.shape == (case[0],)
        assert np.array_equal(y, (torch.tensor(inp['g']) * torch.from_numpy(inp['x'])).numpy())
        assert np.array_equal(y, (np.float64(inp['g']) * inp['x'].astype(np.float64)).astype(np.float32))      # 24 x 24 bits: exact in float64


# ---------------------------------------------------------------------------------------------------------------- 3. the bar discriminates
@pytest.mark.parametrize('name', list(lc.WRONG_KERNELS))
def test_the_bar_fails_a_wrong_kernel(name):
    family, case = lc.WRONG_KERNELS[name]
    cases, inputs, ref_fn, cpu_fn, chain_fn = lc.FAMILIES[family]
    assert case in cases, (name, case)
    inp = inputs(case)
    ref, cpu = ref_fn(inp), cpu_fn(inp)
    assert not lc.hold(lc.case_id(case) + ' [right]', chain_fn(inp), cpu, ref)
    bad = lc.hold(lc.case_id(case) + f' [{name}]', chain_fn(inp, name), cpu, ref)
    assert bad, (name, lc.case_id(case))


def test_wrong_kernel_list_covers_the_defects_the_tests_were_written_for():
    assert len(lc.WRONG_KERNELS) >= 11 and {f for f, _ in lc.WRONG_KERNELS.values()} == {'image', 'token', 'reg', 'kld', 'adam'}


# ---------------------------------------------------------------------------------------------------------------- 4. repeated dims
@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_reg_loss_entry_points_reject_a_repeated_dimension(lib):
    """pure host code: every call below is refused before any launch, the pointers are never dereferenced"""
    from arvae_amd import ops
    fake = ctypes.c_void_p(256)

    def call(dims, ldz=10, ldl=6):
        arr = (ctypes.c_int32 * len(dims))(*dims)
        return lib.arvae_reg_loss(fake, fake, 8, fake, fake, 8, ldz, ldl, arr, len(dims), 10.0, 1.0, fake, fake, fake, None)
    assert call((1, 2, 1)) == -1 and b'dim 1 listed twice' in lib.arvae_last_error_string()
    assert call((0, 5, 3, 5)) == -1 and b'dim 5 listed twice' in lib.arvae_last_error_string()
    assert call(tuple(range(8)) + tuple(range(8)), 16, 16) == -1 and b'listed twice' in lib.arvae_last_error_string()
    assert call((1, 6)) == -1 and b'outside' in lib.arvae_last_error_string()          # (the range check still comes first)
    z, lab = torch.zeros(8, 10), torch.zeros(8, 6)
    with pytest.raises(ValueError, match='listed twice'):
        ops.reg_loss(z, lab, (1, 2, 1), 10.0, 1.0)
    with pytest.raises(ValueError, match='listed twice'):
        ops.reg_loss(z, lab, [3, 3], 10.0, 1.0)
    with pytest.raises(RuntimeError, match='GPU only'):                                  # distinct dims get as far as the device check
        ops.reg_loss(z, lab, (1, 2), 10.0, 1.0)


def test_image_executor_rejects_repeated_reg_dims(lib):
    """the finishing step of a data-parallel pass validates reg_dims before its first launch: a model descriptor with a repeated
    dimension is ARVAE_E_INVALID there (descriptor built on the CPU, as test_abi.py does)"""
    from arvae_amd.fused import FusedImageVAE
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.optim import FlatAdam
    torch.manual_seed(0)
    model = DspritesVAE()
    fused = FusedImageVAE(model, FlatAdam(model.parameters(), lr=1e-4), (1, 2, 3, 2), 4.0, 10.0, 1.0, 'bernoulli')
    d = fused.descriptor()
    fake = ctypes.c_void_p(256)
    rc = lib.arvae_image_vae_finish(ctypes.byref(d), 8, fake, 6, None, fake, fake, 16, 2.0, fake, fake, fake, fake, fake, None)
    assert rc == -1 and b'reg dim 2 listed twice' in lib.arvae_last_error_string()
    d.reg_dims[3] = 9
    rc = lib.arvae_image_vae_finish(ctypes.byref(d), 8, fake, 6, None, fake, fake, 16, 2.0, fake, fake, fake, fake, fake, None)
    assert rc == -1 and b'outside' in lib.arvae_last_error_string()

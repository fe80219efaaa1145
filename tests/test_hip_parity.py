"""Parity of the HIP path (through the C-ABI) against the CPU oracle and the reference goldens.
Needs a real MI355X: run with `pytest -m gpu`."""
import json
import os
import subprocess
import time
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arvae_amd import synthetic as syn

pytestmark = pytest.mark.gpu

from oracle import image_vae as o_vae          # noqa: E402
from oracle import losses as o_losses          # noqa: E402
from oracle import step as o_step              # noqa: E402

# the diagnostic build of the library (csrc/diag.h: its environment switches are live; the product library has none)
DIAG_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ar-vae_amd', 'libarvae_hip_diag.so')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def G(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def close(a, b, rtol=1e-4, atol=0.0):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else b
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------- reg loss (G1)
@pytest.mark.parametrize('n', [7, 64, 512])
def test_reg_loss_golden(golden_dir, dev, n):
    from arvae_amd import ops
    g = G(golden_dir, 'reg_loss.npz')
    x = g[f'n{n}/x']
    for tag in ('cont', 'ties'):
        a = g[f'n{n}/a_{tag}']
        for delta in (1.0, 10.0):
            for gamma in (1.0, 10.0):
                key = f'n{n}_{tag}_d{delta:g}_g{gamma:g}'
                z = torch.from_numpy(np.stack([x * 0, x], 1)).to(dev).requires_grad_(True)
                lab = torch.from_numpy(np.stack([a * 0, a], 1)).to(dev)
                loss = ops.reg_loss(z, lab, (1,), gamma, delta)
                loss.backward()
                close(loss, g[f'{key}/loss'], rtol=1e-5)
                close(z.grad[:, 1], g[f'{key}/grad'], rtol=1e-4, atol=3e-7 * gamma * delta)
                assert float(z.grad[:, 0].abs().max()) == 0.0


def test_reg_loss_multi_dim_and_row_block(dev):
    """all dims in one launch == sum of closed forms; row-block (data-parallel) form == global."""
    from arvae_amd import ops
    rs = np.random.RandomState(3)
    n, zd = 200, 10
    z = rs.standard_normal((n, zd)).astype(np.float32)
    lab = rs.randint(0, 4, (n, 6)).astype(np.float32)
    dims = (1, 2, 3, 4, 5)
    want_l, want_g = 0.0, np.zeros((n, zd))
    for d in dims:
        l, gr = o_losses.reg_loss_closed_form(z[:, d], lab[:, d], 10.0, 1.0)
        want_l += l
        want_g[:, d] = gr
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    lt = torch.from_numpy(lab).to(dev)
    loss = ops.reg_loss(zt, lt, dims, 10.0, 1.0)
    (3.0 * loss).backward()
    close(loss, want_l, rtol=1e-5)
    close(zt.grad, 3.0 * want_g, rtol=1e-4, atol=1e-6)
    # two shards, gathered columns
    parts, grads = [], []
    for sl in (slice(0, 120), slice(120, 200)):
        zs = torch.from_numpy(z[sl]).to(dev).requires_grad_(True)
        ls = torch.from_numpy(lab[sl]).to(dev)
        part = ops.reg_loss(zs, ls, dims, 10.0, 1.0, z_cols=zt.detach(), lab_cols=lt)
        part.backward()
        parts.append(float(part))
        grads.append(zs.grad.cpu().numpy())
    close(sum(parts), want_l, rtol=1e-5)
    close(np.concatenate(grads), want_g, rtol=1e-4, atol=1e-6)


def test_reg_loss_large_batch(dev):
    """global batch 4096 (8 x 512): more columns than one LDS chunk."""
    from arvae_amd import ops
    rs = np.random.RandomState(4)
    n = 4096
    z = rs.standard_normal((n, 10)).astype(np.float32)
    lab = rs.randint(0, 32, (n, 6)).astype(np.float32)
    want_l, want_g = o_losses.reg_loss_closed_form(z[:, 4], lab[:, 4], 10.0, 1.0)
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    loss = ops.reg_loss(zt, torch.from_numpy(lab).to(dev), (4,), 10.0, 1.0)
    loss.backward()
    close(loss, want_l, rtol=2e-5)
    close(zt.grad[:, 4], want_g, rtol=1e-3, atol=1e-7)


# ---------------------------------------------------------------- latent head / KL (G2)
@pytest.mark.parametrize('b,z', [(8, 10), (64, 10), (32, 32)])
def test_latent_head_golden(golden_dir, dev, b, z):
    from arvae_amd import ops
    g = G(golden_dir, 'latent_head.npz')
    mu, ls, eps = (g[f'b{b}_z{z}/{k}'] for k in ('mu', 'log_std', 'eps'))
    w = torch.from_numpy(syn.normal_noise((b, z), seed=99)).to(dev)
    for c in (0.0, 25.0):
        for beta in (4.0, 0.001):
            key = f'b{b}_z{z}_c{c:g}_beta{beta:g}'
            mt = torch.from_numpy(mu).to(dev).requires_grad_(True)
            lt = torch.from_numpy(ls).to(dev).requires_grad_(True)
            sigma, zt = ops.latent_head(mt, lt, torch.from_numpy(eps).to(dev))
            kld = ops.kld_loss(mt, sigma, beta, torch.tensor([c], device=dev))
            (kld.sum() + (zt * w).sum()).backward()
            close(zt, g[f'b{b}_z{z}/z'], rtol=0, atol=1e-5)
            close(sigma, g[f'b{b}_z{z}/sigma'], rtol=1e-5)
            close(kld, g[f'{key}/kld'], rtol=1e-5)
            close(mt.grad, g[f'{key}/dmu'], rtol=1e-4, atol=1e-6)
            close(lt.grad, g[f'{key}/dls'], rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------- reconstruction terms (G3)
@pytest.mark.parametrize('b,hw', [(4, 64), (16, 28)])
def test_image_recon_golden(golden_dir, dev, b, hw):
    from arvae_amd import ops
    g = G(golden_dir, 'recon.npz')
    rs = np.random.RandomState(b * hw)
    logits = (3.0 * rs.standard_normal((b, 1, hw, hw))).astype(np.float32)
    logits.ravel()[::97] = 0.0
    x = (rs.random_sample((b, 1, hw, hw)) < 0.2).astype(np.float32)
    if hw == 28:
        x = (x * rs.random_sample(x.shape)).astype(np.float32)
    for dist in ('bernoulli', 'gaussian'):
        lt = torch.from_numpy(logits).to(dev).requires_grad_(True)
        loss, acc = ops.image_recon(lt, torch.from_numpy(x).to(dev), dist)
        loss.backward()
        close(loss, g[f'b{b}_{hw}_{dist}/loss'], rtol=1e-5)
        close(lt.grad.cpu().numpy().ravel()[::131], g[f'b{b}_{hw}_{dist}/dlogits_samp'], rtol=1e-4, atol=1e-7)
        close(lt.grad.double().abs().sum(), g[f'b{b}_{hw}_{dist}/dlogits_abs_sum'], rtol=1e-5)
        close(acc, g[f'b{b}_{hw}/acc'], rtol=1e-6)


@pytest.mark.parametrize('b', [5, 32])
def test_token_recon_golden(golden_dir, dev, b):
    from arvae_amd import ops
    g = G(golden_dir, 'recon.npz')
    w = torch.from_numpy(g[f'ce_b{b}/w']).to(dev).requires_grad_(True)
    tgt = torch.from_numpy(g[f'ce_b{b}/tgt']).to(dev)
    ce, acc = ops.token_recon(w, tgt)
    ce.backward()
    close(ce, g[f'ce_b{b}/loss'], rtol=1e-5)
    close(acc, g[f'ce_b{b}/acc'], rtol=1e-6)
    close(w.grad.cpu().numpy().ravel()[::37], g[f'ce_b{b}/dw_samp'], rtol=1e-4, atol=1e-8)


# ---------------------------------------------------------------- links vs torch fp32 on CPU
# (the accuracy bar of the single-channel rows -- chi = 1 here, chi(out) = 1 in DECONV_CASES -- is in
# test_single_channel_links_float64.py: float64 references, linear maps, the batches at which the persistent loops run again)
CONV_CASES = [  # (n, hi, chi, clo, k, s, p, act)
    (3, 64, 1, 32, 4, 2, 1, 'relu'), (5, 32, 32, 32, 4, 2, 1, 'relu'), (9, 8, 32, 32, 4, 2, 1, 'relu'),
    (2, 28, 1, 64, 4, 1, 0, 'selu'), (2, 25, 64, 64, 4, 1, 0, 'selu'), (3, 22, 64, 8, 4, 1, 0, 'selu'),
    # more row-group tiles than CUs: the persistent loop of the row-staged kernel (conv64s.hip), both of its tile shapes
    (47, 25, 64, 64, 4, 1, 0, 'selu'), (70, 22, 64, 8, 4, 1, 0, 'none'), (3, 21, 64, 16, 4, 1, 0, 'relu'),
    # the row-staged kernel with padding: source rows above / below the image (its tiles' scalar row offsets start before the tensor)
    (5, 12, 64, 64, 4, 1, 1, 'relu'), (3, 9, 64, 8, 4, 1, 2, 'selu'),
    # single-channel stride-1 links with 64 channels: the per-wave streaming weight gradient (conv_c1.hip, wgrad_c1w)
    (5, 28, 1, 64, 4, 1, 0, 'none'), (90, 28, 1, 64, 4, 1, 0, 'relu'), (3, 19, 1, 64, 4, 1, 0, 'none'),
]


def _act(name):
    return {'relu': F.relu, 'selu': F.selu, 'none': lambda t: t}[name]


def _act_id(name):
    return {'none': 0, 'relu': 1, 'selu': 2}[name]


@pytest.mark.parametrize('case', CONV_CASES, ids=[str(c) for c in CONV_CASES])
@pytest.mark.parametrize('use_mask', [False, True])
def test_conv_down_vs_torch(dev, case, use_mask):
    """nn.Conv2d forward + all three gradients."""
    from arvae_amd import ops
    n, hi, chi, clo, k, s, p, act = case
    lo = (hi + 2 * p - k) // s + 1
    rs = np.random.RandomState(hi * chi + clo)
    x = rs.standard_normal((n, chi, hi, hi)).astype(np.float32)
    w = (rs.standard_normal((clo, chi, k, k)) * 0.2).astype(np.float32)
    b = rs.standard_normal(clo).astype(np.float32)
    gy = rs.standard_normal((n, clo, lo, lo)).astype(np.float32)
    mask = (rs.random_sample((n, clo, lo, lo)) >= 0.5).astype(np.uint8) if use_mask else None
    xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
    y = _act(act)(F.conv2d(xt, wt, bt, stride=s, padding=p))
    if use_mask:
        y = y * torch.from_numpy(mask).float() * 2.0
    y.backward(torch.from_numpy(gy))
    link = ops.Link(hi, hi, chi, lo, lo, clo, k, k, s, p)
    xd = nhwc(torch.from_numpy(x)).to(dev).requires_grad_(True)
    wd, bd = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b))
    md = None if mask is None else nhwc(torch.from_numpy(mask)).to(dev)
    yd = ops.conv_down(xd, wd, bd, link, _act_id(act), md)
    yd.backward(nhwc(torch.from_numpy(gy)).to(dev))
    tol = dict(rtol=2e-4, atol=2e-4)
    close(nchw(yd), y, **tol)
    close(nchw(xd.grad), xt.grad, **tol)
    close(wd.grad, wt.grad, rtol=2e-4, atol=2e-4 * float(wt.grad.abs().max()))
    close(bd.grad, bt.grad, rtol=2e-4, atol=2e-4 * float(bt.grad.abs().max()))


DECONV_CASES = [  # (n, lo, clo(in), chi(out), k, s, p, act)
    (4, 4, 32, 32, 4, 2, 1, 'relu'), (3, 16, 32, 32, 4, 2, 1, 'relu'), (2, 32, 32, 1, 4, 2, 1, 'none'),
    (2, 19, 8, 64, 4, 1, 0, 'selu'), (2, 22, 64, 64, 4, 1, 0, 'selu'), (3, 25, 64, 1, 4, 1, 0, 'none'),
    (55, 22, 64, 64, 4, 1, 0, 'selu'), (3, 17, 64, 12, 4, 1, 0, 'relu'), (5, 11, 64, 64, 4, 1, 1, 'selu'), (2, 10, 64, 8, 4, 1, 2, 'none'),
    (4, 25, 64, 1, 4, 1, 0, 'none'), (85, 25, 64, 1, 4, 1, 0, 'none'), (2, 14, 64, 1, 4, 1, 0, 'relu'),
]


@pytest.mark.parametrize('case', DECONV_CASES, ids=[str(c) for c in DECONV_CASES])
@pytest.mark.parametrize('use_mask', [False, True])
def test_conv_up_vs_torch(dev, case, use_mask):
    """nn.ConvTranspose2d forward + all three gradients."""
    from arvae_amd import ops
    n, lo, clo, chi, k, s, p, act = case
    hi = (lo - 1) * s - 2 * p + k
    rs = np.random.RandomState(lo * clo + chi)
    x = rs.standard_normal((n, clo, lo, lo)).astype(np.float32)
    w = (rs.standard_normal((clo, chi, k, k)) * 0.2).astype(np.float32)
    b = rs.standard_normal(chi).astype(np.float32)
    gy = rs.standard_normal((n, chi, hi, hi)).astype(np.float32)
    mask = (rs.random_sample((n, chi, hi, hi)) >= 0.5).astype(np.uint8) if use_mask else None
    xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
    y = _act(act)(F.conv_transpose2d(xt, wt, bt, stride=s, padding=p))
    if use_mask:
        y = y * torch.from_numpy(mask).float() * 2.0
    y.backward(torch.from_numpy(gy))
    link = ops.Link(hi, hi, chi, lo, lo, clo, k, k, s, p)
    xd = nhwc(torch.from_numpy(x)).to(dev).requires_grad_(True)
    wd, bd = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b))
    md = None if mask is None else nhwc(torch.from_numpy(mask)).to(dev)
    yd = ops.conv_up(xd, wd, bd, link, _act_id(act), md)
    yd.backward(nhwc(torch.from_numpy(gy)).to(dev))
    tol = dict(rtol=2e-4, atol=2e-4)
    close(nchw(yd), y, **tol)
    close(nchw(xd.grad), xt.grad, **tol)
    close(wd.grad, wt.grad, rtol=2e-4, atol=2e-4 * float(wt.grad.abs().max()))
    close(bd.grad, bt.grad, rtol=2e-4, atol=2e-4 * float(bt.grad.abs().max()))


DENSE_CASES = [(8, 512, 256, (32, 16), (0, 0)), (64, 256, 512, (0, 0), (32, 16)), (5, 2888, 256, (8, 361), (0, 0)),
               (7, 256, 2888, (0, 0), (8, 361)), (33, 10, 256, (0, 0), (0, 0)), (512, 256, 10, (0, 0), (0, 0))]


@pytest.mark.parametrize('case', DENSE_CASES, ids=[str(c) for c in DENSE_CASES])
def test_dense_vs_torch(dev, case):
    """nn.Linear with the NCHW-flatten channel permutation on either side."""
    from arvae_amd import ops
    n, fin, fout, in_perm, out_perm = case
    rs = np.random.RandomState(fin + fout)
    x = rs.standard_normal((n, fin)).astype(np.float32)          # feature order = NCHW flatten
    w = (rs.standard_normal((fout, fin)) * 0.1).astype(np.float32)
    b = rs.standard_normal(fout).astype(np.float32)
    gy = rs.standard_normal((n, fout)).astype(np.float32)
    xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
    y = F.relu(F.linear(xt, wt, bt))
    y.backward(torch.from_numpy(gy))

    def to_mem(t, perm):          # NCHW-flatten feature order -> channels-last memory order
        if perm == (0, 0):
            return t.contiguous()
        c, hw = perm
        return t.reshape(t.shape[0], c, hw).permute(0, 2, 1).reshape(t.shape[0], -1).contiguous()

    def from_mem(t, perm):
        if perm == (0, 0):
            return t
        c, hw = perm
        return t.reshape(t.shape[0], hw, c).permute(0, 2, 1).reshape(t.shape[0], -1)

    link = ops.Link.dense(fin, fout, in_perm=in_perm, out_perm=out_perm)
    xd = to_mem(torch.from_numpy(x), in_perm).to(dev).requires_grad_(True)
    wd, bd = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b))
    yd = ops.dense(xd, wd, bd, link, 1)
    yd.backward(to_mem(torch.from_numpy(gy), out_perm).to(dev))
    close(from_mem(yd.detach().cpu(), out_perm), y, rtol=2e-4, atol=2e-4)
    close(from_mem(xd.grad.cpu(), in_perm), xt.grad, rtol=2e-4, atol=2e-4)
    close(wd.grad, wt.grad, rtol=2e-4, atol=2e-4 * float(wt.grad.abs().max()))
    close(bd.grad, bt.grad, rtol=2e-4, atol=2e-4 * float(bt.grad.abs().max()))


# ---------------------------------------------------------------- Adam
def test_adam_vs_oracle(dev):
    from arvae_amd import ops
    rs = np.random.RandomState(8)
    n = 10007
    p = rs.standard_normal(n).astype(np.float32)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    pad = (n + 3) // 4 * 4
    pd, md, vd, gd = (torch.zeros(pad, device=dev) for _ in range(4))
    pd[:n] = torch.from_numpy(p).to(dev)
    for step in range(1, 4):
        g = (rs.standard_normal(n) * 10 ** rs.uniform(-3, 1)).astype(np.float32)
        p, m, v = o_losses.adam_step(p, g, m, v, step, lr=1e-3)
        gd[:n] = torch.from_numpy(g).to(dev)
        ops.adam_step(pd, gd, md, vd, step, 1e-3)
        # one fp32 ulp of the largest entry as atol: b1*m + (1-b1)*g cancels for some elements
        close(pd[:n], p, rtol=1e-5, atol=2e-7 * float(np.abs(p).max()))
        close(md[:n], m, rtol=1e-5, atol=2e-7 * float(np.abs(m).max()))
        close(vd[:n], v, rtol=1e-5, atol=2e-7 * float(np.abs(v).max()))


# ---------------------------------------------------------------- full steps (G4 / G5)
class DspritesDataset:
    pass


class MorphoMnistDataset:
    pass


IMAGE_CASES = [
    ('dsprites_step_b8.npz', 'dsprites', 8, 1, 1234, 11, 4.0, 0.0, 'bernoulli', None, 1.6),
    ('dsprites_step_b64.npz', 'dsprites', 64, 1, 1234, 12, 4.0, 0.0, 'bernoulli', None, 1.6),
    ('dsprites_step_b8_cap_gauss.npz', 'dsprites', 8, 2, 77, 13, 1.0, 25.0, 'gaussian', None, 1.6),
    ('mnist_step_eval.npz', 'mnist', 8, 3, 4321, 14, 1.0, 0.0, 'bernoulli', None, 0.7),
    ('mnist_step_train.npz', 'mnist', 8, 3, 4321, 15, 1.0, 0.0, 'bernoulli', 21, 0.7),
]


def run_hip_image_step(dev, kind, state, x, lab, eps, beta, cap, dist, masks, train=True, steps=1, fused=True):
    from arvae_amd.image_vae import DspritesVAE, MnistVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    model = DspritesVAE() if kind == 'dsprites' else MnistVAE()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    dims = (1, 2, 3, 4, 5) if kind == 'dsprites' else (1, 2, 3, 4, 5, 6)
    ds = DspritesDataset() if kind == 'dsprites' else MorphoMnistDataset()
    trainer = ImageVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=dims, dec_dist=dist, beta=beta,
                              gamma=10.0, capacity=cap, rand=0, delta=1.0)
    trainer.cuda()
    trainer.use_fused = fused
    model.train() if train else model.eval()
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    out = None
    for _ in range(steps):
        model.push_noise(torch.from_numpy(eps))
        if masks is not None:
            model.push_dropout_masks([nhwc(torch.from_numpy(m)) for m in masks])
        trainer.zero_grad()
        loss, acc = trainer.loss_and_acc_for_batch((xt, lt), 0, 0, train)
        loss.backward()
        grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()}
        trainer.step()
        out = dict(loss=float(loss), acc=float(acc), grads=grads,
                   terms={k: (None if v is None else float(v)) for k, v in trainer.last_terms.items()})
    out['params'] = {k: p.detach().cpu().numpy().copy() for k, p in model.named_parameters()}
    out['model'], out['trainer'] = model, trainer
    return out


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'per_layer'])
@pytest.mark.parametrize('case', IMAGE_CASES, ids=[c[0][:-4] for c in IMAGE_CASES])
def test_image_step_vs_golden_and_oracle(golden_dir, dev, case, fused):
    fname, kind, b, wseed, xseed, eseed, beta, cap, dist, mseed, gain = case
    g = G(golden_dir, fname)
    state = syn.synth_state(o_vae.SHAPES[kind], wseed, gain)
    x, lab = (syn.dsprites_batch if kind == 'dsprites' else syn.mnist_batch)(b, seed=xseed)
    eps = syn.normal_noise((b, o_vae.Z_DIM[kind]), seed=eseed)
    dims = (1, 2, 3, 4, 5) if kind == 'dsprites' else (1, 2, 3, 4, 5, 6)
    masks = None if mseed is None else syn.dropout_masks([(b,) + s for s in o_vae.MNIST_MASK_SHAPES], mseed)
    train = not fname.endswith('eval.npz')
    got = run_hip_image_step(dev, kind, state, x, lab, eps, beta, cap, dist, masks, train=train, fused=fused)
    ref = o_step.image_step(kind, state, x, lab, eps, dims, beta, 10.0, 1.0, capacity=cap, dec_dist=dist, masks=masks)
    # loss terms: north_star tolerance rtol 1e-4 (fp32), against the reference golden AND the oracle
    for src in (g, ref['terms']):
        close(got['terms']['recons'], float(src['recons']), rtol=1e-4)
        close(got['terms']['dist'], float(src['dist']), rtol=1e-4)
        close(got['terms']['reg'], float(src['reg']), rtol=1e-4)
        close(got['loss'], float(src['loss']), rtol=1e-4)
        close(got['acc'], float(src['acc']), rtol=1e-4)
    # gradients: per-tensor norm rtol 1e-3, sampled entries, Adam deltas
    for name in state:
        gr = got['grads'][name].astype(np.float64).ravel()
        gn = float(g[f'gnorm/{name}'])
        close(np.sqrt((gr * gr).sum()), gn, rtol=1e-3)
        idx = syn.sample_indices(name, gr.size)
        close(gr[idx], g[f'gsamp/{name}'], rtol=1e-3, atol=1e-3 * gn / np.sqrt(gr.size) + 1e-7)
        # whole tensor vs the oracle: relative L2 error (a ReLU unit whose pre-activation is ~0 may flip
        # between two fp32 summation orders, which moves a handful of entries by more than 1e-3 each)
        want = ref['grads'][name].astype(np.float64).ravel()
        assert np.linalg.norm(gr - want) <= 2e-3 * np.linalg.norm(want) + 1e-9, name
        d = (got['params'][name].astype(np.float64) - state[name].astype(np.float64)).ravel()
        close(np.sqrt((d * d).sum()), g[f'dnorm/{name}'], rtol=2e-3)


def test_image_forward_latents_vs_golden(golden_dir, dev):
    """z, mu, sigma atol 1e-4 and logits against the goldens (dSprites B=64)."""
    from arvae_amd.image_vae import DspritesVAE
    g = G(golden_dir, 'dsprites_step_b64.npz')
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    x, _ = syn.dsprites_batch(64, seed=1234)
    model = DspritesVAE()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.cuda().train()
    model.push_noise(torch.from_numpy(syn.normal_noise((64, 10), seed=12)))
    with torch.no_grad():
        logits, z_dist, prior, z, z_prior = model(torch.from_numpy(x).to(dev))
    assert logits.shape == (64, 1, 64, 64) and z.shape == (64, 10) and z_prior.shape == (64, 10)
    close(z, g['z'], rtol=0, atol=1e-4)
    close(z_dist.loc, g['mu'], rtol=0, atol=1e-4)
    close(z_dist.scale, g['sigma'], rtol=1e-4, atol=1e-5)
    lg = logits.cpu().numpy().ravel()
    close(lg.astype(np.float64).sum(), g['logits_sum'], rtol=1e-4, atol=1e-2)
    close(lg[syn.sample_indices('logits', lg.size, 64)], g['logits_samp'], rtol=1e-4, atol=1e-4)
    assert float(prior.loc.abs().max()) == 0.0 and float(prior.scale.min()) == 1.0


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'per_layer'])
def test_three_steps_track_oracle(dev, fused):
    """Adam state carried over several steps stays on the oracle's trajectory."""
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 5, 1.6)
    x, lab = syn.dsprites_batch(16, seed=3)
    eps = syn.normal_noise((16, 10), seed=4)
    got = run_hip_image_step(dev, 'dsprites', state, x, lab, eps, 4.0, 0.0, 'bernoulli', None, steps=3, fused=fused)
    cur, adam = state, None
    for step_no in (1, 2, 3):
        ref = o_step.image_step('dsprites', cur, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0, adam_state=adam,
                                step_no=step_no)
        cur, adam = ref['params'], ref['adam']
    close(got['loss'], ref['terms']['loss'], rtol=1e-4)
    for name in state:
        # Adam divides by sqrt(v): an entry whose gradient is ~0 turns a last-bit gradient difference into a visible step
        close(got['params'][name], cur[name], rtol=0, atol=1e-5)


@pytest.mark.parametrize('b', [3, 37, 130, 1100])
def test_image_step_ragged_batches_vs_oracle(dev, b):
    """Batch sizes that leave partial tiles in every kernel (whole-image tiles of 2 / 8 images, 8-row head blocks); 1100
    is past the size where the 8x8 / 4x4 layers switch from their small-tile to their 128-pixel kernels."""
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 9, 1.6)
    x, lab = syn.dsprites_batch(b, seed=50 + b)
    eps = syn.normal_noise((b, 10), seed=60 + b)
    got = run_hip_image_step(dev, 'dsprites', state, x, lab, eps, 4.0, 0.0, 'bernoulli', None)
    ref = o_step.image_step('dsprites', state, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)
    for k in ('recons', 'dist', 'reg', 'loss', 'acc'):
        close(got['loss'] if k == 'loss' else got['acc'] if k == 'acc' else got['terms'][k], float(ref['terms'][k]), rtol=1e-4)
    for name in state:
        gr = got['grads'][name].astype(np.float64).ravel()
        want = ref['grads'][name].astype(np.float64).ravel()
        assert np.linalg.norm(gr - want) <= 2e-3 * np.linalg.norm(want) + 1e-9, name


@pytest.mark.parametrize('b,train', [(37, True), (130, True), (67, False)], ids=['b37_train', 'b130_train', 'b67_eval'])
def test_mnist_step_ragged_batches_vs_oracle(dev, b, train):
    """Morpho-MNIST at batch sizes that leave partial tiles in the wide Linear layers' tile GEMMs (round 6: dense.hip
    wide_gemm_x3_kernel / wide_wgrad_x3_kernel: 64-row tiles with 37 / 3 / 2 live rows, split reductions of 16 / 4 / 8 slices, the
    bf16 planes of the small activations read along a batch that is no multiple of the 32-row chunk) and in the 64-channel conv
    kernels; train mode with explicit keep-masks, eval mode without."""
    state = syn.synth_state(o_vae.SHAPES['mnist'], 3, 0.7)
    x, lab = syn.mnist_batch(b, seed=900 + b)
    eps = syn.normal_noise((b, 16), seed=910 + b)
    masks = syn.dropout_masks([(b,) + s for s in o_vae.MNIST_MASK_SHAPES], 920 + b) if train else None
    got = run_hip_image_step(dev, 'mnist', state, x, lab, eps, 1.0, 0.0, 'bernoulli', masks, train=train)
    ref = o_step.image_step('mnist', state, x, lab, eps, (1, 2, 3, 4, 5, 6), 1.0, 10.0, 1.0, masks=masks)
    _compare_step(got['terms'], got['loss'], got['acc'], got['grads'], ref, 2e-3)
    outs = got['trainer'].last_outputs
    close(outs['z'], ref['terms']['z'], rtol=0, atol=1e-4)
    close(outs['mu'], ref['terms']['mu'], rtol=0, atol=1e-4)


def test_deferred_finishing_step_is_nan_until_backward_and_changes_nothing(dev):
    """ARVAE_VAE_DEFER_FINISH (round 6): a training step leaves the forward pass's finishing launch to the first launch of its
    backward pass.  Between the two calls the loss reads as NaN (poisoned by the forward pass's last launch: a caller that looks too
    early sees it, not a stale number); after backward() it is the value of the step that finishes inside the forward pass (another
    summation order over 512 instead of 1024 threads: rtol 1e-6), and the gradients are the same sums (the last decoder layer's
    weight gradient is summed over 255 instead of 256 slabs, the rider takes a workgroup: relative L2 1e-6; the rest bit for bit)."""
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    b = 512
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 5, 1.6)
    x, lab = syn.dsprites_batch(b, seed=77)
    eps = torch.from_numpy(syn.normal_noise((b, 10), seed=78))
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    got = {}
    for defer in (True, False):
        model = DspritesVAE()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        trainer = ImageVAETrainer(DspritesDataset(), model, lr=1e-4, reg_type=('all',), reg_dim=(1, 2, 3, 4, 5), beta=4.0, gamma=10.0,
                                  capacity=0.0, rand=0, delta=1.0)
        trainer.cuda()
        trainer.defer_loss_finish = defer
        model.train()
        model.push_noise(eps)
        trainer.zero_grad()
        loss, acc = trainer.loss_and_acc_for_batch((xt, lt), 0, 0, True)
        early = float(loss.detach())
        assert np.isnan(early) == defer                          # poisoned until backward() / final at once
        loss.backward()
        torch.cuda.synchronize()
        got[defer] = (float(loss.detach()), float(acc), {k: float(v) for k, v in trainer.last_terms.items()},
                      trainer.optimizer.grad_arena.clone())
        with torch.no_grad():                                    # an evaluation pass never defers
            model.push_noise(eps)
            l_eval, _ = trainer.loss_and_acc_for_batch((xt, lt), 0, 1, False)
            assert np.isfinite(float(l_eval))
    np.testing.assert_allclose(got[True][0], got[False][0], rtol=1e-6)
    np.testing.assert_allclose(got[True][1], got[False][1], rtol=1e-6)
    for k in ('recons', 'dist', 'reg'):
        np.testing.assert_allclose(got[True][2][k], got[False][2][k], rtol=1e-6)
    ga, gb = got[True][3].double(), got[False][3].double()
    assert float((ga - gb).norm()) <= 1e-6 * float(gb.norm())
    assert float((got[True][3] != got[False][3]).float().mean()) < 0.01        # (deconv4's 512 weights + bias of ~500 k entries)


def _full_batch_grads(dev, scale, seed=7):
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, seed, 1.6)
    model = DspritesVAE()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = ImageVAETrainer(DspritesDataset(), model, lr=1e-4, reg_type=('all',), reg_dim=(1, 2, 3, 4, 5), beta=4.0,
                              gamma=10.0, capacity=0.0, rand=0, delta=1.0)
    trainer.cuda()
    model.train()
    x, lab = syn.dsprites_batch(512, seed=1234)
    model.push_noise(torch.from_numpy(syn.normal_noise((512, 10), seed=1)))
    trainer.zero_grad()
    loss, _ = trainer.loss_and_acc_for_batch((torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)), 0, 0, True)
    (loss * scale).backward()
    return float(loss), trainer.optimizer.grad_arena.detach().clone()


def test_full_batch_properties(dev):
    """BASELINE's batch (512), size-independent properties: the step is bit-reproducible (no atomics anywhere) and the
    whole backward pass is linear in the upstream gradient (it is folded into the first kernels' loads)."""
    l1, g1 = _full_batch_grads(dev, 1.0)
    l2, g2 = _full_batch_grads(dev, 1.0)
    assert l1 == l2 and torch.equal(g1, g2)
    _, g3 = _full_batch_grads(dev, 3.0)
    assert np.isfinite(l1) and float(g1.abs().max()) > 0
    close(g3, 3.0 * g1, rtol=2e-5, atol=1e-6 * float(g1.abs().max()))


@pytest.mark.parametrize('batch', [512, 200])
def test_clustered_latent_block_handoffs_under_load(dev, batch):
    """The clustered latent block (csrc/midcluster.hip) hands activations between workgroups through memory inside ONE launch
    (sc1 stores, a counter, sc1 loads): a stale or torn read would show as a changed bit somewhere.  300 forward + backward
    passes over the same weights, inputs and noise -- the exchanged buffers are the same addresses every pass, so every
    consumer's caches are warm with the previous pass's bytes -- while a second stream keeps the memory system busy with an
    uneven load (copies of changing sizes): the loss, z, every saved latent tensor's checksum and the whole gradient arena must
    be bit-identical in every pass.  batch 200: seven clusters, the last one with eight valid rows (cross-XCD clusters:
    the cluster count is not a multiple of eight)."""
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 7, 1.6)
    model = DspritesVAE()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = ImageVAETrainer(DspritesDataset(), model, lr=1e-4, reg_type=('all',), reg_dim=(1, 2, 3, 4, 5), beta=4.0,
                              gamma=10.0, capacity=0.0, rand=0, delta=1.0)
    trainer.cuda()
    model.train()
    x, lab = syn.dsprites_batch(batch, seed=1234)
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    eps = torch.from_numpy(syn.normal_noise((batch, 10), seed=1)).to(dev)
    side = torch.cuda.Stream()
    junk_a, junk_b = torch.empty(48 << 20, device=dev), torch.empty(48 << 20, device=dev)
    first = None
    for it in range(300):
        with torch.cuda.stream(side):                          # uneven competing traffic: 4 .. 192 MB copies
            n = (1 + (it * 7) % 48) << 20
            junk_b[:n].copy_(junk_a[:n])
        model.push_noise(eps)
        trainer.zero_grad()
        loss, _ = trainer.loss_and_acc_for_batch((xt, lt), 0, 0, True)
        trainer.backward(loss)
        got = torch.cat([loss.detach().reshape(1), trainer.optimizer.grad_arena.detach()])
        if first is None:
            first = got.clone()
            assert torch.isfinite(first).all() and float(first[1:].abs().max()) > 0
        else:
            assert torch.equal(got, first), f'pass {it}: {int((got != first).sum())} words differ'
    torch.cuda.synchronize()


def _conv32_maps(dev, hi_np, lo_np, w_np, b_np):
    """the three maps of a 32-channel k4 s2 p1 link through the per-layer C-ABI (weights split and maxima taken in the caller's
    workspace): forward Conv2d of hi, forward ConvTranspose2d of lo, weight / bias gradient of the Conv2d for upstream `lo`"""
    from arvae_amd import ops
    n, size = hi_np.shape[0], lo_np.shape[1]
    hi_d, lo_d, w_d, b_d = (torch.from_numpy(a).to(dev) for a in (hi_np, lo_np, w_np, b_np))
    link = ops.Link(2 * size, 2 * size, 32, size, size, 32, 4, 4, 2, 1)
    got = {'down': ops.link_down(link, n, ops._operand(hi_d), w_d, b_d, ops.ACT_NONE, None),
           'up': ops.link_up(link, n, ops._operand(lo_d), w_d, b_d, ops.ACT_NONE, None)}
    dw, db = torch.zeros_like(w_d), torch.zeros_like(b_d)
    ops.link_wgrad(link, n, ops._operand(lo_d), ops._operand(hi_d), dw, db, 1)
    got.update(dw=dw, db=db)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _conv32_maps_float64(hi_np, lo_np, w_np, b_np):
    hi = torch.from_numpy(hi_np).double().permute(0, 3, 1, 2)
    lo = torch.from_numpy(lo_np).double().permute(0, 3, 1, 2)
    w = torch.from_numpy(w_np).double().requires_grad_(True)
    b = torch.from_numpy(b_np).double().requires_grad_(True)
    down = F.conv2d(hi, w, b, stride=2, padding=1)
    up = F.conv_transpose2d(lo, w, b, stride=2, padding=1)
    down.backward(lo)                                    # dW, db of the Conv2d for the upstream gradient `lo`
    return {'down': down.detach().permute(0, 2, 3, 1).numpy(), 'up': up.detach().permute(0, 2, 3, 1).numpy(),
            'dw': w.grad.numpy(), 'db': b.grad.numpy()}


@pytest.mark.parametrize('size', [16, 8, 4])
def test_scaled_two_term_fp16_kernels_hold_fp32_accuracy_vs_float64(dev, size):
    """The 32-channel conv kernels run the fp16 MFMA on scaled two-term operands (three partial products, fp32 accumulation;
    splitmath.h): against a float64 reference of the same three maps their relative L2 error stays below 5e-7, i.e. fp32
    rounding noise -- the bar the three-term bf16 generation (rounds 1-3) and the fp32-MFMA generation before it were held to."""
    rs = np.random.RandomState(11)
    n = 24 if size == 16 else 64
    hi_np = rs.standard_normal((n, 2 * size, 2 * size, 32)).astype(np.float32)
    lo_np = rs.standard_normal((n, size, size, 32)).astype(np.float32)
    w_np = (rs.standard_normal((32, 32, 4, 4)) * 0.1).astype(np.float32)
    b_np = rs.standard_normal(32).astype(np.float32)
    got, ref = _conv32_maps(dev, hi_np, lo_np, w_np, b_np), _conv32_maps_float64(hi_np, lo_np, w_np, b_np)
    for k in ('down', 'up', 'dw', 'db'):
        err = np.linalg.norm(got[k].astype(np.float64) - ref[k]) / np.linalg.norm(ref[k])
        assert err < 5e-7, (k, err)


def test_conv32_scaling_is_exact_and_survives_outliers(dev):
    """What the per-tensor power-of-two scales must guarantee.  (1) Results do not depend on the magnitude of the operands:
    a tensor times 2^k gives bit for bit the result times 2^k (gradients of 1e-7 are as good as activations of 1e+3).
    (2) A tensor whose maximum sits far above its bulk (one value 10^4 times the rest: the low terms of the bulk then fall
    into the fp16 subnormal range, absolute error <= 2^-39 of the maximum) still meets the float64 bar relative to the result's
    norm, and the outputs the outlier does not reach keep an error of a few 1e-7 relative to their own norm."""
    rs = np.random.RandomState(5)
    n, size = 16, 16
    hi_np = np.maximum(rs.standard_normal((n, 32, 32, 32)), 0).astype(np.float32)      # ReLU-like: half zeros
    lo_np = rs.standard_normal((n, 16, 16, 32)).astype(np.float32)
    w_np = (rs.standard_normal((32, 32, 4, 4)) * 0.1).astype(np.float32)
    b0 = np.zeros(32, np.float32)
    base = _conv32_maps(dev, hi_np, lo_np, w_np, b0)
    for k_hi, k_lo, k_w in ((-23, 0, 0), (9, -30, 0), (0, 0, -7), (-12, 14, 5)):
        s_hi, s_lo, s_w = np.float32(2.0 ** k_hi), np.float32(2.0 ** k_lo), np.float32(2.0 ** k_w)
        got = _conv32_maps(dev, hi_np * s_hi, lo_np * s_lo, w_np * s_w, b0)
        np.testing.assert_array_equal(got['down'], base['down'] * (s_hi * s_w))
        np.testing.assert_array_equal(got['up'], base['up'] * (s_lo * s_w))
        np.testing.assert_array_equal(got['dw'], base['dw'] * (s_hi * s_lo))
    hi_out, lo_out = hi_np.copy(), lo_np.copy()
    hi_out[3, 7, 9, 11] = 1.0e4 * np.abs(hi_np).max()
    lo_out[5, 2, 3, 4] = -1.0e4 * np.abs(lo_np).max()
    got, ref = _conv32_maps(dev, hi_out, lo_out, w_np, b0), _conv32_maps_float64(hi_out, lo_out, w_np, b0)
    for k in ('down', 'up', 'dw', 'db'):
        err = np.linalg.norm(got[k].astype(np.float64) - ref[k]) / np.linalg.norm(ref[k])
        assert err < 5e-7, (k, err)
    # and what the outlier does NOT touch keeps its accuracy: output pixels away from it, against float64, relative to THEIR norm
    far = np.ones(got['down'].shape[:3], bool)
    far[3, 2:6, 3:7] = False
    err = np.linalg.norm(got['down'][far].astype(np.float64) - ref['down'][far]) / np.linalg.norm(ref['down'][far])
    assert err < 5e-6, err


# ---------------------------------------------------------------- MeasureVAE (G6 / G7)
class _FolkDataset:
    """the attributes MeasureVAE / MeasureVAETrainer read from the reference's FolkNBarDataset"""
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


def test_measure_attributes_golden(golden_dir, dev):
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer, build_measure_tables
    from oracle import attributes as o_attr
    g = G(golden_dir, 'attributes.npz')
    tables = build_measure_tables(_FolkDataset(), dev)
    lut = syn.measure_tables()
    for got, want in zip(tables, lut):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    from arvae_amd import ops
    w = torch.tensor([0.20, 1, 2, 0.5, 2, 1, 0.67, 1, 2, 0.5, 2, 1, 0.25, 1, 2, 0.5, 2, 1, 0.67, 1, 2, 0.5, 2, 1],
                     dtype=torch.float64).float()
    out = ops.measure_attributes(torch.from_numpy(g['score']).to(dev), tables, w.to(dev), float(w.sum()))
    close(out, g['attr'], rtol=1e-6, atol=1e-7)
    big = syn.measure_batch(4096, seed=77)
    out = ops.measure_attributes(torch.from_numpy(big).to(dev), tables, w.to(dev), float(w.sum()))
    close(out, o_attr.attribute_labels(big, *lut), rtol=1e-6, atol=1e-7)


def test_gru_cell_vs_torch(dev):
    """dense + gate kernels reproduce torch.nn.GRUCell forward and gradients."""
    from arvae_amd import ops
    rs = np.random.RandomState(5)
    b, fin, hid = 37, 138, 128
    cell = torch.nn.GRUCell(fin, hid)
    x = torch.from_numpy(rs.standard_normal((b, fin)).astype(np.float32)).requires_grad_(True)
    h = torch.from_numpy(rs.standard_normal((b, hid)).astype(np.float32)).requires_grad_(True)
    gy = torch.from_numpy(rs.standard_normal((b, hid)).astype(np.float32))
    y = cell(x, h)
    y.backward(gy)
    prm = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in cell.named_parameters()}
    xd, hd = x.detach().to(dev).requires_grad_(True), h.detach().to(dev).requires_grad_(True)
    gi = ops.dense(xd, prm['weight_ih'], prm['bias_ih'], ops.Link.dense(fin, 3 * hid), 0)
    gh = ops.dense(hd, prm['weight_hh'], prm['bias_hh'], ops.Link.dense(hid, 3 * hid), 0)
    yd = ops.gru_gates(gi, gh, hd)
    yd.backward(gy.to(dev))
    close(yd, y, rtol=1e-5, atol=1e-6)
    close(xd.grad, x.grad, rtol=1e-4, atol=1e-6)
    close(hd.grad, h.grad, rtol=1e-4, atol=1e-6)
    for k, v in cell.named_parameters():
        close(prm[k].grad, v.grad, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('rows,hid,steps', [(37, 128, 24), (16, 64, 6), (5, 32, 4), (602, 128, 4), (1301, 64, 3)])
def test_gru_sequence_vs_torch(dev, rows, hid, steps):
    """whole-sequence GRU kernels (both directions in one launch, initial state, ragged row count) reproduce a
    bidirectional torch.nn.GRU layer: outputs, input-projection / initial-state gradients, W_hh / b_hh gradients.
    (The kernels own 4, 8 or 16 batch rows per workgroup, whichever fills the chip in one round: 37, 602 and 1301 rows x 2
    directions select the three widths on a 256-CU device.)"""
    from arvae_amd import ops
    rs = np.random.RandomState(15)
    fin = 10
    torch.manual_seed(15)                # (nn.GRU draws its parameters from torch's generator: pinned, whatever ran before)
    gru = torch.nn.GRU(fin, hid, 1, bidirectional=True)
    x = torch.from_numpy(rs.standard_normal((steps, rows, fin)).astype(np.float32)).requires_grad_(True)
    h0 = torch.from_numpy(rs.standard_normal((2, rows, hid)).astype(np.float32)).requires_grad_(True)
    gy = torch.from_numpy(rs.standard_normal((steps, rows, 2 * hid)).astype(np.float32))
    gfin = torch.from_numpy(rs.standard_normal((rows, 2 * hid)).astype(np.float32))
    y, hn = gru(x, h0)
    ((y * gy).sum() + (torch.cat((hn[0], hn[1]), 1) * gfin).sum()).backward()
    prm = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in gru.named_parameters()}
    xd = x.detach().to(dev).requires_grad_(True)
    hd = h0.detach().to(dev).requires_grad_(True)
    dirs = []
    for d, suf in enumerate(('', '_reverse')):
        gi = ops.dense(xd.view(steps * rows, fin), prm['weight_ih_l0' + suf], prm['bias_ih_l0' + suf],
                       ops.Link.dense(fin, 3 * hid), 0).view(steps, rows, 3 * hid)
        dirs.append((gi, prm['weight_hh_l0' + suf], prm['bias_hh_l0' + suf], hd[d], d == 1))
    yd, fin = ops.gru_sequence(steps, dirs)
    ((yd * gy.to(dev)).sum() + (fin * gfin.to(dev)).sum()).backward()
    close(yd, y, rtol=1e-5, atol=2e-6)
    close(fin[:, :hid], hn[0], rtol=1e-5, atol=2e-6)
    close(fin[:, hid:], hn[1], rtol=1e-5, atol=2e-6)
    close(xd.grad, x.grad, rtol=1e-4, atol=2e-6)
    close(hd.grad, h0.grad, rtol=1e-4, atol=2e-6)
    for k, v in gru.named_parameters():                  # (sums over steps x rows terms, against torch's own fp32 sums)
        close(prm[k].grad, v.grad, rtol=1e-4, atol=2e-5 if rows < 100 else 2e-4)


@pytest.mark.parametrize('w_scale,h_scale,g_scale', [(1.0, 1.0, 1.0), (40.0, 6000.0, 1.0), (1.0, 1.0, 1e-9), (1.0, 1.0, 1e+6),
                                                      (3000.0, 1.0, 1e-4)])
def test_fp16_recurrences_scale_themselves(dev, w_scale, h_scale, g_scale):
    """both recurrences multiply on the fp16 MFMA with scales taken from the data (round 5: per-wave scales for W_hh, the workgroup's
    largest |h0| for the state, per batch row and step for the backward pass's gradients): recurrent weights beyond 255 and initial
    states beyond 4094 overflowed the fixed scales of round 4, and upstream gradients of 1e-9 or 1e+6 would leave the
    useful range of a fixed gradient scale.  Against a FLOAT64 nn.GRU the outputs and every gradient keep fp32 accuracy relative
    to their largest element, and nothing is inf or nan."""
    from arvae_amd import ops
    rows, hid, steps, fin = 21, 128, 12, 10
    torch.manual_seed(3)
    rs = np.random.RandomState(33)
    gru = torch.nn.GRU(fin, hid, 1, bidirectional=True)
    with torch.no_grad():
        for k, v in gru.named_parameters():
            if 'weight_hh' in k:
                v.mul_(w_scale)
    x = torch.from_numpy(rs.standard_normal((steps, rows, fin)).astype(np.float32))
    h0 = torch.from_numpy((h_scale * rs.standard_normal((2, rows, hid))).astype(np.float32))
    gy = torch.from_numpy((g_scale * rs.standard_normal((steps, rows, 2 * hid))).astype(np.float32))
    g64 = torch.nn.GRU(fin, hid, 1, bidirectional=True).double()
    g64.load_state_dict({k: v.double() for k, v in gru.state_dict().items()})
    x64, h64 = x.double().requires_grad_(True), h0.double().requires_grad_(True)
    y64, _ = g64(x64, h64)
    (y64 * gy.double()).sum().backward()
    # torch's own fp32 CPU layer on the same problem: the yardstick (saturated gates make some of these draws ill-conditioned)
    x32, h32 = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    y32, _ = gru(x32, h32)
    (y32 * gy).sum().backward()
    prm = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in gru.named_parameters()}
    xd, hd = x.to(dev).requires_grad_(True), h0.to(dev).requires_grad_(True)
    dirs = []
    for d, suf in enumerate(('', '_reverse')):
        gi = ops.dense(xd.view(steps * rows, fin), prm['weight_ih_l0' + suf], prm['bias_ih_l0' + suf],
                       ops.Link.dense(fin, 3 * hid), 0).view(steps, rows, 3 * hid)
        dirs.append((gi, prm['weight_hh_l0' + suf], prm['bias_hh_l0' + suf], hd[d], d == 1))
    yd, _ = ops.gru_sequence(steps, dirs)
    (yd * gy.to(dev)).sum().backward()
    assert bool(torch.isfinite(yd).all())

    def rel(got, want):
        return float((got.detach().cpu().double() - want.detach()).abs().max()) / max(float(want.detach().abs().max()), 1e-300)

    assert rel(yd, y64) <= max(2e-6, 3 * rel(y32, y64)), ('y', rel(yd, y64), rel(y32, y64))
    for name, got, ref32, want in [('x', xd.grad, x32.grad, x64.grad), ('h0', hd.grad, h32.grad, h64.grad)] + \
            [(k, prm[k].grad, dict(gru.named_parameters())[k].grad, v.grad) for k, v in g64.named_parameters()]:
        assert bool(torch.isfinite(got).all()), name
        assert rel(got, want) <= max(2e-5, 5 * rel(ref32, want)), (name, rel(got, want), rel(ref32, want))


@pytest.mark.parametrize('seed', [0, 6, 8])
def test_fp16_forward_recurrence_holds_fp32_accuracy_vs_float64(dev, seed):
    """the forward recurrence multiplies on the fp16 MFMA (scaled two-term operands, three products: gru_seq.hip) and the backward one
    on the three-term bf16 split: against a FLOAT64 bidirectional nn.GRU (24 steps, 37 rows, H = 128, non-zero initial states) the
    outputs stay as close as torch's own fp32 CPU layer does (measured over twelve draws: 2.3-3.1e-7 against 3.0-5.8e-7,
    tools/probes/gru_error.py), and the gradients agree with the float64 ones to a few 1e-6 of their largest element."""
    from arvae_amd import ops
    rows, hid, steps, fin = 37, 128, 24, 10
    torch.manual_seed(seed)
    rs = np.random.RandomState(15 + seed)
    gru = torch.nn.GRU(fin, hid, 1, bidirectional=True)
    x = torch.from_numpy(rs.standard_normal((steps, rows, fin)).astype(np.float32))
    h0 = torch.from_numpy(rs.standard_normal((2, rows, hid)).astype(np.float32))
    gy = torch.from_numpy(rs.standard_normal((steps, rows, 2 * hid)).astype(np.float32))
    with torch.no_grad():
        y32, _ = gru(x, h0)
    g64 = torch.nn.GRU(fin, hid, 1, bidirectional=True).double()
    g64.load_state_dict({k: v.double() for k, v in gru.state_dict().items()})
    x64, h64 = x.double().requires_grad_(True), h0.double().requires_grad_(True)
    y64, _ = g64(x64, h64)
    (y64 * gy.double()).sum().backward()
    prm = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in gru.named_parameters()}
    xd, hd = x.to(dev).requires_grad_(True), h0.to(dev).requires_grad_(True)
    dirs = []
    for d, suf in enumerate(('', '_reverse')):
        gi = ops.dense(xd.view(steps * rows, fin), prm['weight_ih_l0' + suf], prm['bias_ih_l0' + suf],
                       ops.Link.dense(fin, 3 * hid), 0).view(steps, rows, 3 * hid)
        dirs.append((gi, prm['weight_hh_l0' + suf], prm['bias_hh_l0' + suf], hd[d], d == 1))
    yd, _ = ops.gru_sequence(steps, dirs)
    (yd * gy.to(dev)).sum().backward()
    e_hip = float((yd.detach().cpu().double() - y64.detach()).abs().max())
    e_cpu = float((y32.double() - y64.detach()).abs().max())
    assert e_hip <= 1.5 * e_cpu + 1e-7 and e_hip <= 1e-6, (e_hip, e_cpu)
    for name, got, want in [('x', xd.grad, x64.grad), ('h0', hd.grad, h64.grad)] + \
            [(k, prm[k].grad, v.grad) for k, v in g64.named_parameters()]:
        err = float((got.detach().cpu().double() - want).abs().max()) / float(want.abs().max())
        assert err <= 5e-6, (name, err)


@pytest.mark.parametrize('rows,hid,steps,fin', [(256, 128, 24, 10), (37, 128, 24, 256), (9, 32, 5, 12)])
def test_merged_bidirectional_projection_vs_torch(dev, rows, hid, steps, fin):
    """Both directions' input projections as ONE product (ops.dense_pair over weights / biases / gradient buffers laid out
    back to back, as the trainer's arena holds them: MeasureVAE.arena_parameters) feeding ONE sequence launch that reads its
    two gi blocks with a row stride and returns ONE gradient for the projection: outputs, final states (written by the launch:
    arvae_gru_seq_t.h_fin) and every gradient against a bidirectional torch.nn.GRU layer."""
    from arvae_amd import ops
    rs = np.random.RandomState(23)
    torch.manual_seed(23)
    gru = torch.nn.GRU(fin, hid, 1, bidirectional=True)
    x = torch.from_numpy(rs.standard_normal((steps, rows, fin)).astype(np.float32)).requires_grad_(True)
    gy = torch.from_numpy(rs.standard_normal((steps, rows, 2 * hid)).astype(np.float32))
    gfin = torch.from_numpy(rs.standard_normal((rows, 2 * hid)).astype(np.float32))
    y, hn = gru(x)
    ((y * gy).sum() + (torch.cat((hn[0], hn[1]), 1) * gfin).sum()).backward()
    ref = dict(gru.named_parameters())
    # the four input-projection tensors side by side in one buffer (values and gradients), everything else on its own
    nw, nb = 3 * hid * fin, 3 * hid
    flat = torch.zeros(2 * nw + 2 * nb, device=dev)
    gflat = torch.zeros_like(flat)
    prm = {}
    for i, (name, off, shape) in enumerate((('weight_ih_l0', 0, (3 * hid, fin)), ('weight_ih_l0_reverse', nw, (3 * hid, fin)),
                                            ('bias_ih_l0', 2 * nw, (3 * hid,)), ('bias_ih_l0_reverse', 2 * nw + nb, (3 * hid,)))):
        n = int(np.prod(shape))
        flat[off:off + n].copy_(ref[name].detach().reshape(-1))
        p = torch.nn.Parameter(flat[off:off + n].view(shape))
        p.grad = gflat[off:off + n].view(shape)
        prm[name] = p
    for name in ('weight_hh_l0', 'bias_hh_l0', 'weight_hh_l0_reverse', 'bias_hh_l0_reverse'):
        prm[name] = ref[name].detach().clone().to(dev).requires_grad_(True)
    xd = x.detach().to(dev).requires_grad_(True)
    gi_all = ops.dense_pair(xd.view(steps * rows, fin), prm['weight_ih_l0'], prm['bias_ih_l0'], prm['weight_ih_l0_reverse'],
                            prm['bias_ih_l0_reverse'])
    assert gi_all is not None and gi_all.shape == (steps * rows, 6 * hid)
    yd, fin_d = ops.gru_sequence(steps, [(None, prm['weight_hh_l0'], prm['bias_hh_l0'], None, False),
                                         (None, prm['weight_hh_l0_reverse'], prm['bias_hh_l0_reverse'], None, True)],
                                 merged_gi=gi_all.view(steps, rows, -1))
    ((yd * gy.to(dev)).sum() + (fin_d * gfin.to(dev)).sum()).backward()
    close(yd, y, rtol=1e-5, atol=2e-6)
    close(fin_d[:, :hid], hn[0], rtol=1e-5, atol=2e-6)
    close(fin_d[:, hid:], hn[1], rtol=1e-5, atol=2e-6)
    close(xd.grad, x.grad, rtol=1e-4, atol=2e-6)
    for k, v in gru.named_parameters():
        # sums over steps x rows terms (6144 at the encoder's size) in two different fp32 orders: whole-tensor relative L2, and
        # no single entry further off than a few ulps of the tensor's largest
        got, want = prm[k].grad.detach().cpu().double(), v.grad.double()
        assert float((got - want).norm()) <= 1e-5 * float(want.norm()), k
        close(prm[k].grad, v.grad, rtol=1e-4, atol=1e-5 * float(want.abs().max()) + 3e-5)
    # not adjacent -> the caller is told to run the layers one by one
    lone = torch.nn.Parameter(prm['weight_ih_l0_reverse'].detach().clone())
    assert ops.dense_pair(xd.view(steps * rows, fin), prm['weight_ih_l0'], prm['bias_ih_l0'], lone, prm['bias_ih_l0_reverse']) is None


def test_gru_sequence_constant_input(dev):
    """one input projection reused at every step (the beat RNN's constant input) and no initial state."""
    from arvae_amd import ops
    rs = np.random.RandomState(16)
    rows, hid, steps = 19, 128, 4
    gru = torch.nn.GRU(1, hid, 1)
    x1 = torch.from_numpy(rs.standard_normal((rows, 1)).astype(np.float32)).requires_grad_(True)
    gy = torch.from_numpy(rs.standard_normal((steps, rows, hid)).astype(np.float32))
    y, _ = gru(x1[None].expand(steps, -1, -1))
    (y * gy).sum().backward()
    prm = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in gru.named_parameters()}
    xd = x1.detach().to(dev).requires_grad_(True)
    gi = ops.dense(xd, prm['weight_ih_l0'], prm['bias_ih_l0'], ops.Link.dense(1, 3 * hid), 0)
    yd, _ = ops.gru_sequence(steps, [(gi, prm['weight_hh_l0'], prm['bias_hh_l0'], None, False)])
    (yd * gy.to(dev)).sum().backward()
    close(yd, y, rtol=1e-5, atol=2e-6)
    close(xd.grad, x1.grad, rtol=1e-4, atol=2e-6)
    for k, v in gru.named_parameters():
        close(prm[k].grad, v.grad, rtol=1e-4, atol=2e-5)


def test_measure_sequence_path_matches_stepwise(dev, monkeypatch):
    """the whole-sequence MeasureVAE path and the one-launch-per-step path give the same losses and gradients
    (teacher-forced and free-running decoder, dropout masks on)."""
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    b = 21
    score = torch.from_numpy(syn.measure_batch(b, seed=18)).to(dev)
    eps = torch.from_numpy(syn.normal_noise((b, 32), seed=19))
    gen = torch.Generator().manual_seed(3)
    masks = [(torch.rand(24, b, 256, generator=gen) >= 0.5).to(torch.uint8),
             (torch.rand(4, b, 128, generator=gen) >= 0.5).to(torch.uint8),
             (torch.rand(24, b, 128, generator=gen) >= 0.5).to(torch.uint8)]
    for teacher in (True, False):
        res = {}
        for mode in ('0', '1'):
            monkeypatch.setenv('ARVAE_GRU_STEPWISE', mode)
            torch.manual_seed(11)
            ds = _FolkDataset()
            model = MeasureVAE(ds, 10, 2, 2, 128, 0.5, 32, 2, 128, 0.5, False, 'folk')
            trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001,
                                        gamma=1.0, capacity=0.0, rand=0, delta=10.0)
            trainer.cuda()
            model.train()
            model.decoder.teacher_forcing_prob = 1.0 if teacher else 0.0
            model.push_noise(eps)
            model.encoder.push_dropout_mask(masks[0].to(dev))
            model.decoder.push_dropout_masks(masks[1].to(dev), masks[2].to(dev))
            trainer.zero_grad()
            loss, acc = trainer.loss_and_acc_for_batch((score, score), 0, 0, True)
            loss.backward()
            res[mode] = (float(loss), float(acc), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
        close(res['0'][0], res['1'][0], rtol=1e-5)
        close(res['0'][1], res['1'][1], rtol=1e-6)
        for k, gstep in res['1'][2].items():
            gseq = res['0'][2][k]
            assert float((gseq - gstep).norm()) <= 2e-4 * float(gstep.norm()) + 1e-9, (teacher, k)


@pytest.mark.parametrize('b,dropout,hid,big', [(256, 0.5, 128, False), (21, 0.0, 128, False), (37, 0.5, 64, False), (1501, 0.5, 128, False),
                                               (2101, 0.0, 64, False), (64, 0.5, 128, True), (45, 0.0, 64, True),
                                               (2053, 0.5, 128, False), (1029, 0.0, 64, False)])
def test_tick_free_run_tokens_match_stepwise(dev, monkeypatch, b, dropout, hid, big):
    """the one-launch free-running tick decoder feeds itself the same notes as the launch-per-tick pass.
    big: initial tick states of ~1e4 and recurrent tick weights of ~350 -- beyond what the FIXED fp16 operand scales of round 4 could
    hold (4094 / 255: inf, then nan); the kernel takes its scales from the data since round 5.
    (2053 rows at hidden 128 and 1029 at hidden 64 are the kernel's 16 and 8 rows per workgroup, five rows in the last one: with
    1501 / 128, 2101 / 64 and the small batches, all three widths at both hidden sizes; hidden 32: test_measure_layers_gpu.py)"""
    from arvae_amd.measure_vae import MeasureVAE
    from gru_cases import rows_per_wg
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if b in (2053, 1029):                                     # the cases named for a width run it, on this device
        want = 16 if b == 2053 else 8
        assert rows_per_wg(b, 1, cus) == want and b % want == 5, \
            f'{b} rows on {cus} CUs run {rows_per_wg(b, 1, cus)} rows per workgroup: this case is written for {want} (256 CUs)'
    torch.manual_seed(23)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, hid, dropout, 32, 2, hid, dropout, False, 'folk').cuda().train()
    with torch.no_grad():                                     # spread the logits so that the argmax varies
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.3)
        if big:
            model.decoder.beat_emb_to_tick_rnn_hidden[0].weight.mul_(20000.0)
            for name in ('weight_hh_l0', 'weight_ih_l1', 'weight_hh_l1'):
                getattr(model.decoder.rnn_tick, name).mul_(4000.0)
            assert float(model.decoder.rnn_tick.weight_hh_l0.abs().max()) > 255.0
    model.decoder.teacher_forcing_prob = 0.0
    score = torch.from_numpy(syn.measure_batch(b, seed=28)).to(dev)
    eps = torch.from_numpy(syn.normal_noise((b, 32), seed=29))
    gen = torch.Generator().manual_seed(4)
    masks = [(torch.rand(24, b, 2 * hid, generator=gen) >= 0.5).to(torch.uint8).to(dev),
             (torch.rand(4, b, hid, generator=gen) >= 0.5).to(torch.uint8).to(dev),
             (torch.rand(24, b, hid, generator=gen) >= 0.5).to(torch.uint8).to(dev)]
    out = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('ARVAE_TICK_STEPWISE', mode)
        model.push_noise(eps)
        if dropout > 0:
            model.encoder.push_dropout_mask(masks[0])
            model.decoder.push_dropout_masks(masks[1], masks[2])
        with torch.no_grad():
            weights, samples, *_ = model(score, score, train=True)
        out[mode] = (weights, samples)
    assert out['0'][1].shape == (b, 1, 24) and out['0'][1].dtype == torch.int64
    assert len(torch.unique(out['1'][1])) > 3                 # a non-trivial token stream
    assert torch.equal(out['0'][1], out['1'][1])
    close(out['0'][0], out['1'][0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('rows,fin,fout,act', [(6144, 128, 384, 0), (2050, 138, 384, 0), (2311, 10, 384, 0),
                                               (6144, 128, 35, 1), (2048, 256, 130, 2)])
def test_dense_long_batch_vs_torch(dev, rows, fin, fout, act):
    """Linear layers over thousands of rows (whole-sequence GEMMs) run on the LDS-staged rows-GEMM kernels:
    forward, data gradient and the row-sliced weight / bias gradient, elementwise within rtol=1e-4 (atol 1e-5 / 2e-4) of a
    float64 torch reference, with each activation.  That bound sees an indexing mistake, not a lost split term:
    test_split_kernels_float64.py holds the same kernels to fp32 accuracy."""
    from arvae_amd import ops
    rs = np.random.RandomState(rows + fin)
    x = torch.from_numpy(rs.standard_normal((rows, fin)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((fout, fin)) / np.sqrt(fin)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(fout).astype(np.float32))
    gy = torch.from_numpy(rs.standard_normal((rows, fout)).astype(np.float32))
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    pre = xr @ wr.t() + br
    y = [pre, torch.relu(pre), torch.nn.functional.selu(pre)][act]
    (y * gy.double()).sum().backward()
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    yd = ops.dense(xd, wd, bd, ops.Link.dense(fin, fout), act)
    (yd * gy.to(dev)).sum().backward()
    close(yd, y, rtol=1e-4, atol=1e-5)
    close(xd.grad, xr.grad, rtol=1e-4, atol=1e-5)
    close(wd.grad, wr.grad, rtol=1e-4, atol=2e-4)
    close(bd.grad, br.grad, rtol=1e-4, atol=2e-4)


def test_embedding_concat_argmax(dev):
    from arvae_amd import ops
    rs = np.random.RandomState(6)
    table = torch.from_numpy(rs.standard_normal((35, 10)).astype(np.float32))
    idx = torch.from_numpy(rs.randint(0, 35, (9, 24)).astype(np.int64))
    gy = torch.from_numpy(rs.standard_normal((24, 9, 10)).astype(np.float32))
    tt = table.clone().requires_grad_(True)
    ref = tt[idx].permute(1, 0, 2)
    ref.backward(gy)
    td = table.to(dev).requires_grad_(True)
    out = ops.embed(idx.to(dev), td, time_major=True)
    out.backward(gy.to(dev))
    close(out, ref, rtol=0, atol=0)
    close(td.grad, tt.grad, rtol=1e-6, atol=1e-6)
    a = torch.from_numpy(rs.standard_normal((7, 10)).astype(np.float32)).to(dev).requires_grad_(True)
    b = torch.from_numpy(rs.standard_normal((7, 128)).astype(np.float32)).to(dev).requires_grad_(True)
    c = ops.concat_cols(a, b)
    lo, hi = ops.split_cols(c, 100)
    (lo.sum() * 2 + hi.sum() * 3).backward()
    close(c, torch.cat((a, b), 1).detach(), rtol=0, atol=0)
    assert float(a.grad.min()) == 2.0 and float(b.grad[:, :90].max()) == 2.0 and float(b.grad[:, 90:].min()) == 3.0
    w = torch.tensor([[0., 0., 0.], [1., 5., 5.], [2., 1., 0.]], device=dev)
    assert ops.row_argmax(w).tolist() == [0, 1, 0]              # lowest index on ties


@pytest.mark.parametrize('batch,dim', [(256, 768), (37, 384), (5, 132)])
def test_wide_lookup_tables(dev, batch, dim):
    """lookups of a per-vocabulary PROJECTION table (rows of hundreds of columns: the encoder's layer-0 input projection of
    both directions applied to the embedding table once, MeasureVAE Encoder._first_layer_by_lookup) and the segment sums that
    take the per-position gradients back to the table's rows (embed_bwd_wide_kernel), against torch indexing; a non-leaf
    table (the usual case: it is computed from parameters) and a leaf one with a gradient buffer to add into."""
    from arvae_amd import ops
    rs = np.random.RandomState(31)
    vocab, steps = 35, 24
    table = torch.from_numpy(rs.standard_normal((vocab, dim)).astype(np.float32))
    idx = torch.from_numpy(rs.randint(0, vocab, (batch, steps)).astype(np.int64))
    gy = torch.from_numpy(rs.standard_normal((steps, batch, dim)).astype(np.float32))
    tt = table.clone().double().requires_grad_(True)
    ref = tt[idx].permute(1, 0, 2)
    ref.backward(gy.double())
    base = table.to(dev).requires_grad_(True)
    out = ops.embed(idx.to(dev), base * 1.0, time_major=True)           # non-leaf table
    out.backward(gy.to(dev))
    close(out, ref.float(), rtol=0, atol=0)
    assert float((base.grad.cpu().double() - tt.grad).norm()) <= 2e-6 * float(tt.grad.norm())
    leaf = table.to(dev).requires_grad_(True)
    leaf.grad = torch.ones_like(leaf)                                   # an existing buffer: the gradient is ADDED
    ops.embed(idx.to(dev), leaf, time_major=True).backward(gy.to(dev))
    assert float((leaf.grad.cpu().double() - 1.0 - tt.grad).norm()) <= 2e-6 * float(tt.grad.norm())


MEASURE_CASES = [('measure_step_tf.npz', 5, 31, True, True), ('measure_step_free.npz', 5, 32, False, True),
                 ('measure_step_eval.npz', 6, 33, False, False)]


@pytest.mark.parametrize('case', MEASURE_CASES, ids=[c[0][:-4] for c in MEASURE_CASES])
def test_measure_step_vs_golden_and_oracle(golden_dir, dev, case):
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    from oracle import attributes as o_attr
    from oracle import measure_vae as o_mvae
    fname, sseed, eseed, teacher, train = case
    g = G(golden_dir, fname)
    state = syn.synth_state(o_mvae.shapes(), 4)
    state['decoder.tick_emb_to_note_emb.0.bias'] = state['decoder.tick_emb_to_note_emb.0.bias'] + np.float32(0.5)
    state['decoder.tick_emb_to_note_emb.0.weight'] = state['decoder.tick_emb_to_note_emb.0.weight'] * np.float32(3.0)
    score = syn.measure_batch(16, seed=sseed)
    eps = syn.normal_noise((16, 32), seed=eseed)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 128, 0.0, 32, 2, 128, 0.0, False, 'folk')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0,
                                capacity=0.0, rand=0, delta=10.0)
    trainer.cuda()
    model.train() if train else model.eval()
    model.decoder.teacher_forcing_prob = 1.0 if teacher else 0.0
    model.push_noise(torch.from_numpy(eps))
    st = torch.from_numpy(score).to(dev)
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((st, st), 0, 0, train)
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()}
    trainer.step()
    attr = o_attr.attribute_labels(score, *syn.measure_tables())
    ref = o_step.measure_step(state, score, eps, attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, teacher)
    for src in (g, ref['terms']):
        close(trainer.last_terms['recons'], float(src['recons']), rtol=1e-4)
        close(trainer.last_terms['dist'], float(src['dist']), rtol=1e-4)
        close(trainer.last_terms['reg'], float(src['reg']), rtol=1e-4)
        close(loss, float(src['loss']), rtol=1e-4)
        close(acc, float(src['acc']), rtol=1e-4)
    with torch.no_grad():
        model.push_noise(torch.from_numpy(eps))
        model.decoder.teacher_forcing_prob = 1.0 if teacher else 0.0
    for name in state:
        gr = grads[name].astype(np.float64).ravel()
        gn = float(g[f'gnorm/{name}'])
        close(np.sqrt((gr * gr).sum()), gn, rtol=2e-3)
        want = ref['grads'][name].astype(np.float64).ravel()
        assert np.linalg.norm(gr - want) <= 3e-3 * np.linalg.norm(want) + 1e-9, name
        d = (model.state_dict()[name].cpu().numpy().astype(np.float64) - state[name].astype(np.float64)).ravel()
        close(np.sqrt((d * d).sum()), g[f'dnorm/{name}'], rtol=3e-3)


def test_measure_forward_outputs_vs_golden(golden_dir, dev):
    """weights, samples, z, mu, sigma of the free-running decoder against the golden."""
    from arvae_amd.measure_vae import MeasureVAE
    from oracle import measure_vae as o_mvae
    g = G(golden_dir, 'measure_step_free.npz')
    state = syn.synth_state(o_mvae.shapes(), 4)
    state['decoder.tick_emb_to_note_emb.0.bias'] = state['decoder.tick_emb_to_note_emb.0.bias'] + np.float32(0.5)
    state['decoder.tick_emb_to_note_emb.0.weight'] = state['decoder.tick_emb_to_note_emb.0.weight'] * np.float32(3.0)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 128, 0.0, 32, 2, 128, 0.0, False, 'folk')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.cuda().train()
    model.decoder.teacher_forcing_prob = 0.0
    model.push_noise(torch.from_numpy(syn.normal_noise((16, 32), seed=32)))
    score = torch.from_numpy(syn.measure_batch(16, seed=5)).to(dev)
    with torch.no_grad():
        weights, samples, z_dist, prior, z, z_prior = model(score, score, train=True)
    assert weights.shape == (16, 24, 35) and samples.shape == (16, 1, 24) and samples.dtype == torch.int64
    np.testing.assert_array_equal(samples.cpu().numpy(), g['samples'])
    close(z, g['z'], rtol=0, atol=1e-4)
    close(z_dist.loc, g['mu'], rtol=0, atol=1e-4)
    close(z_dist.scale, g['sigma'], rtol=1e-4, atol=1e-5)
    w = weights.cpu().numpy()
    close(w[0], g['weights_row0'], rtol=1e-4, atol=1e-5)
    close(w.ravel()[syn.sample_indices('weights', w.size, 128)], g['weights_samp'], rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------- data-parallel path on one GPU
@pytest.mark.parametrize('fused', [False, True], ids=['per_layer', 'executor'])
def test_graphed_measure_step_matches_eager(dev, fused):
    """HIP-graph replay of the MeasureVAE forward + backward (arvae_amd.graphed) against the eager step: same kernels
    in the same order, so loss and gradients are bit-identical (dropout off, fixed noise buffer, coin pinned).  Both the per-layer
    path (a hundred launches: what the trainers replay under data parallelism) and the whole-model executor's two calls."""
    from arvae_amd.graphed import GraphedStep
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    ds = _FolkDataset()
    torch.manual_seed(0)
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.0, 16, 2, 64, 0.0, False, 'folk')
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0,
                                capacity=0.0, rand=0, delta=10.0)
    trainer.cuda()
    trainer.use_fused_step = fused
    model.train()
    b = 32
    model.encoder.static_eps = torch.from_numpy(syn.normal_noise((b, 16), seed=3)).to(dev)
    score = torch.from_numpy(syn.measure_batch(b, seed=8)).to(dev)
    other = torch.from_numpy(syn.measure_batch(b, seed=9)).to(dev)
    try:
        graphed = GraphedStep(trainer, (other, other))           # captured on different data than it is replayed on
        for forced in (True, False):
            model.decoder.teacher_forcing_prob = 2.0 if forced else -1.0
            trainer.zero_grad()
            loss, _ = trainer.loss_and_acc_for_batch((score, score), 0, 1, True)
            loss.backward()
            want_loss, want_grad = float(loss), trainer.optimizer.grad_arena.clone()
            graphed.prob = 2.0 if forced else -1.0
            got_loss, _ = graphed((score, score))
            torch.cuda.synchronize()
            assert float(got_loss) == want_loss
            assert torch.equal(trainer.optimizer.grad_arena, want_grad)
    finally:
        type(model.encoder).static_eps = None
        model.encoder.static_eps = None


def test_measure_epoch_loop_replays_graphs(dev):
    """Trainer.loss_and_acc_on_epoch of the MeasureVAE trainer replays captured graphs for full batches and runs the
    odd-sized last batch eagerly; the weights after the epoch equal those of an all-eager epoch (dropout off, fixed noise
    buffer, teacher forcing pinned on)."""
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    b = 32
    batches = [torch.from_numpy(syn.measure_batch(n, seed=40 + i)).to(dev) for i, n in enumerate((b, b, b, 20))]
    loader = [(x, x) for x in batches]
    final = {}
    for replay in (True, False):
        ds = _FolkDataset()
        torch.manual_seed(0)
        model = MeasureVAE(ds, 10, 2, 2, 64, 0.0, 16, 2, 64, 0.0, False, 'folk')
        trainer = MeasureVAETrainer(ds, model, lr=1e-3, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0,
                                    capacity=0.0, rand=0, delta=10.0)
        assert trainer.use_graph_replay
        trainer.use_graph_replay = replay
        trainer.use_fused_step = False        # the per-layer path (what data-parallel steps run): the whole-model executor is not replayed
        trainer.cuda()
        model.train()
        model.decoder.teacher_forcing_prob = 2.0
        try:
            # one noise buffer for every batch size: rows [0, n) are used
            noise = torch.from_numpy(syn.normal_noise((b, 16), seed=3)).to(dev)
            losses = []
            for x in loader:
                model.encoder.static_eps = noise[:x[0].shape[0]].contiguous() if x[0].shape[0] != b else noise
                l, _ = trainer.loss_and_acc_on_epoch([x], epoch_num=0, train=True)
                losses.append(l)
        finally:
            type(model.encoder).static_eps = None
            model.encoder.static_eps = None
        assert (getattr(trainer, '_graphed', None) is not None) == replay
        final[replay] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()})
    for a, c in zip(final[True][0], final[False][0]):
        close(a, c, rtol=1e-6)
    for k, v in final[False][1].items():
        assert torch.equal(final[True][1][k], v), k


def test_data_parallel_path_single_rank_rccl(dev):
    """world_size 1 over RCCL: the all-gather / all-reduce code path runs on the GPU and must give the same
    loss and gradients as the plain single-process step."""
    import subprocess
    import sys
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for extra in ([], ['--force-dp']):
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '3', '--warmup', '1', '--batch', '64',
                            '--min-seconds', '0', '--no-cpu-baseline'] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert lines, (r.stdout[-1000:], r.stderr[-2000:])
        outs.append(json.loads(lines[-1]))
    a, b = (o['config']['final_loss'] for o in outs)
    assert abs(a - b) <= 2e-3 * abs(a), (a, b)     # eps differs per run only through the shared torch seed -> identical draws


# ---------------------------------------------------------------- BASELINE.json's full batch sizes, HIP vs the oracle
def _compare_step(got_terms, got_loss, got_acc, got_grads, ref, grad_tol):
    for k in ('recons', 'dist', 'reg'):
        close(got_terms[k], float(ref['terms'][k]), rtol=1e-4)
    close(got_loss, float(ref['terms']['loss']), rtol=1e-4)
    close(got_acc, float(ref['terms']['acc']), rtol=1e-4)
    for name, want in ref['grads'].items():
        gr = got_grads[name].astype(np.float64).ravel()
        want = want.astype(np.float64).ravel()
        close(np.linalg.norm(gr), np.linalg.norm(want), rtol=1e-3)
        assert np.linalg.norm(gr - want) <= grad_tol * np.linalg.norm(want) + 1e-9, name


def _compare_headline_golden(g, terms, loss, acc, grads, z, mu, sigma=None):
    """a step at one of BASELINE.json's batch sizes against the REFERENCE's own outputs (tests/golden/make_goldens.py
    gen_headline_steps: loss terms rtol 1e-4, the kept rows of z / mu atol 1e-4 and their whole-tensor sums, per-tensor
    gradient norms rtol 1e-3, sampled gradient entries)"""
    for k in ('recons', 'dist', 'reg'):
        close(float(terms[k]), float(g[k]), rtol=1e-4)
    close(float(loss), float(g['loss']), rtol=1e-4)
    close(float(acc), float(g['acc']), rtol=1e-4)
    rows = g['z'].shape[0]
    for name, got in (('z', z), ('mu', mu), ('sigma', sigma)):
        if got is None:
            continue
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        close(got[:rows], g[name], rtol=1e-4 if name == 'sigma' else 0, atol=1e-5 if name == 'sigma' else 1e-4)
        close(got.astype(np.float64).sum(), float(g[f'{name}_sum']), rtol=1e-4, atol=1e-4 * got.shape[0])
        close(np.abs(got.astype(np.float64)).sum(), float(g[f'{name}_abs_sum']), rtol=1e-4)
    for name, gr in grads.items():
        gr = gr.astype(np.float64).ravel()
        gn = float(g[f'gnorm/{name}'])
        close(np.linalg.norm(gr), gn, rtol=1e-3)
        idx = syn.sample_indices(name, gr.size)
        # sampled entries: rtol 2e-3 + 2e-3 of the tensor's RMS (an entry fed by a ReLU unit whose pre-activation is ~0 moves by
        # that much between two fp32 summation orders: the same allowance as the whole-tensor relative L2 of the oracle tests)
        close(gr[idx], g[f'gsamp/{name}'], rtol=2e-3, atol=2e-3 * gn / np.sqrt(gr.size) + 1e-7)


def test_dsprites_step_at_baseline_batch_512_vs_oracle(golden_dir, dev):
    """BASELINE.json configs[1]: the headline batch, full training step against the oracle (loss terms rtol 1e-4, z / mu
    atol 1e-4, every gradient tensor by norm and relative L2, the weights after Adam) and against the reference's own
    outputs at this size (tests/golden/dsprites_step_b512.npz)."""
    b = 512
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    x, lab = syn.dsprites_batch(b, seed=1234)
    eps = syn.normal_noise((b, 10), seed=1)
    got = run_hip_image_step(dev, 'dsprites', state, x, lab, eps, 4.0, 0.0, 'bernoulli', None)
    ref = o_step.image_step('dsprites', state, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)
    _compare_step(got['terms'], got['loss'], got['acc'], got['grads'], ref, 2e-3)
    outs = got['trainer'].last_outputs
    close(outs['z'], ref['terms']['z'], rtol=0, atol=1e-4)
    close(outs['mu'], ref['terms']['mu'], rtol=0, atol=1e-4)
    close(outs['sigma'], ref['terms']['sigma'], rtol=1e-4, atol=1e-6)
    g = G(golden_dir, 'dsprites_step_b512.npz')
    _compare_headline_golden(g, got['terms'], got['loss'], got['acc'], got['grads'], outs['z'], outs['mu'], outs['sigma'])
    for name in state:
        d_got = (got['params'][name].astype(np.float64) - state[name]).ravel()
        d_ref = (ref['params'][name].astype(np.float64) - state[name]).ravel()
        close(np.linalg.norm(d_got), np.linalg.norm(d_ref), rtol=2e-3)
        close(np.linalg.norm(d_got), float(g[f'dnorm/{name}']), rtol=2e-3)


def _shared_device_reference():
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    x, lab = syn.dsprites_batch(512, seed=1234)
    eps = syn.normal_noise((512, 10), seed=1)
    return o_step.image_step('dsprites', state, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)


def _check_shared_device_result(path, ref):
    r = np.load(path)
    terms = dict(zip([str(k) for k in r['terms_keys']], [float(v) for v in r['terms_vals']]))
    grads = {k[2:]: r[k] for k in r.files if k.startswith('g/')}
    _compare_step(terms, float(r['loss']), float(r['acc']), grads, ref, 2e-3)
    return r


def test_two_processes_share_the_device(dev, tmp_path):
    """Two fresh processes train at the headline batch on cuda:0 AT THE SAME TIME, 200 steps each: both finish, no hand-off of
    the clustered latent block gives up (its 16-workgroup clusters form from whichever workgroups are resident: tickets,
    csrc/midcluster.hip), every repetition reproduces the first bit for bit, and the step is the oracle's.  (Through round 4 a
    cluster's members were fixed by blockIdx: two processes could each hold half of every cluster and spin forever.)"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shared_device_worker.py')
    sync = tmp_path / 'sync'
    sync.mkdir()
    outs = [str(tmp_path / f'p{i}.npz') for i in range(2)]
    procs = [subprocess.Popen([sys.executable, worker, o, '200', str(sync), '0'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for o in outs]
    try:
        deadline = time.time() + 300
        while len([f for f in os.listdir(sync) if f.startswith('ready_')]) < 2:
            assert all(p.poll() is None for p in procs), [p.communicate()[1][-1500:] for p in procs if p.poll() is not None]
            assert time.time() < deadline, 'the workers did not come up'
            time.sleep(0.05)
        (sync / 'go').write_text('')
        for p in procs:
            _, err = p.communicate(timeout=600)
            assert p.returncode == 0, err[-2000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    ref = _shared_device_reference()
    for o in outs:
        r = _check_shared_device_result(o, ref)
        assert bool(r['same']), 'a repetition under a shared device differed from the first one'


def test_handoff_that_never_completes_raises_instead_of_hanging(dev, tmp_path):
    """The diagnostic library drops ONE arrival of the forward latent block's first hand-off (ARVAE_MIDC_DROP_ARRIVAL): the
    launch must end by itself (bounded poll), the trainer's status check must raise RuntimeError, and the same trainer must
    carry on with the row kernels and produce the oracle's step."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shared_device_worker.py')
    out = str(tmp_path / 'dropped.npz')
    r = subprocess.run([sys.executable, worker, out, '3', '-', '1'], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ARVAE_LIB=DIAG_LIB, ARVAE_MIDC_DROP_ARRIVAL='1'))
    assert r.returncode == 0, r.stderr[-2000:]
    res = _check_shared_device_result(out, _shared_device_reference())
    assert 'hand-off' in str(res['raised']) and bool(res['same'])
    assert float(res['first_seconds']) < 30.0


def test_epoch_with_a_failed_handoff_is_repeated_from_intact_weights(dev, tmp_path):
    """a failed in-launch hand-off used to be seen once per epoch, AFTER Adam had applied up to an epoch of
    undefined gradients.  arvae_adam_step now reads the status word itself and withholds the update; Trainer.loss_and_acc_on_epoch
    repeats the epoch on the row kernels.  Three batches of 512 with the first pass's arrival dropped (diagnostic library) must
    end with the weights, the step count and the epoch mean of an undisturbed run."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shared_device_worker.py')
    outs = {}
    for name, env in (('clean', {}), ('dropped', dict(ARVAE_LIB=DIAG_LIB, ARVAE_MIDC_DROP_ARRIVAL='1'))):
        outs[name] = str(tmp_path / f'{name}.npz')
        r = subprocess.run([sys.executable, worker, outs[name], '3', '-', '2'], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        assert ('repeating the epoch' in r.stdout) == (name == 'dropped'), r.stdout[-1500:]
    clean, dropped = np.load(outs['clean']), np.load(outs['dropped'])
    assert int(clean['step_count']) == 3 and int(dropped['step_count']) == 3
    assert bool(dropped['no_cluster']) and not bool(clean['no_cluster'])
    np.testing.assert_allclose(dropped['mean_loss'], clean['mean_loss'], rtol=1e-5)
    # row kernels against cluster kernels: the same fp32-accurate arithmetic in another summation order, through three Adam
    # updates of 1e-3 (an update is at most lr per entry whatever the gradient)
    assert np.abs(dropped['params'] - clean['params']).max() <= 2e-4
    assert np.abs(dropped['params'] - clean['params']).mean() <= 1e-6


def test_mnist_step_at_baseline_batch_1024_vs_oracle(golden_dir, dev):
    """BASELINE.json configs[2]: Morpho-MNIST AR-VAE at batch 1024 in TRAIN mode with explicit dropout keep-masks (the five
    Dropout(0.5) layers of imagevae/mnist_vae.py:16-47), conv64.hip path with its full grid of tiles; against the oracle
    and against the reference's own outputs at this size (tests/golden/mnist_step_train_b1024.npz)."""
    b = 1024
    state = syn.synth_state(o_vae.SHAPES['mnist'], 3, 0.7)
    x, lab = syn.mnist_batch(b, seed=4321)
    eps = syn.normal_noise((b, 16), seed=15)
    masks = syn.dropout_masks([(b,) + s for s in o_vae.MNIST_MASK_SHAPES], 21)
    got = run_hip_image_step(dev, 'mnist', state, x, lab, eps, 1.0, 0.0, 'bernoulli', masks)
    ref = o_step.image_step('mnist', state, x, lab, eps, (1, 2, 3, 4, 5, 6), 1.0, 10.0, 1.0, masks=masks)
    _compare_step(got['terms'], got['loss'], got['acc'], got['grads'], ref, 2e-3)
    outs = got['trainer'].last_outputs
    close(outs['z'], ref['terms']['z'], rtol=0, atol=1e-4)
    close(outs['mu'], ref['terms']['mu'], rtol=0, atol=1e-4)
    _compare_headline_golden(G(golden_dir, 'mnist_step_train_b1024.npz'), got['terms'], got['loss'], got['acc'], got['grads'],
                             outs['z'], outs['mu'], outs.get('sigma'))


@pytest.mark.parametrize('dropout', [0.0, 0.5], ids=['p0', 'p0.5'])
@pytest.mark.parametrize('teacher', [True, False], ids=['teacher_forced', 'free_running'])
def test_measure_step_at_baseline_batch_256_vs_oracle(golden_dir, dev, teacher, dropout):
    """BASELINE.json configs[4]: MeasureVAE (H = 128, Z = 32, V = 35) training step at batch 256, forward AND backward,
    teacher-forced and free-running; the sampled notes must equal the oracle's (the output layer is given a positive top-1
    margin as in the golden cases, SURVEY.md section 7 'top-1 tie-breaking').  dropout 0.5 is the configuration bench.py
    times: the three inter-layer keep-masks (encoder layer 0 outputs, beat / tick layer-0 hidden states) are explicit and
    go through oracle.measure_vae.forward(..., masks=...) and the HIP path's mask queues alike."""
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    from oracle import attributes as o_attr
    from oracle import measure_vae as o_mvae
    b = 256
    state = syn.synth_state(o_mvae.shapes(), 4)
    state['decoder.tick_emb_to_note_emb.0.bias'] = state['decoder.tick_emb_to_note_emb.0.bias'] + np.float32(0.5)
    state['decoder.tick_emb_to_note_emb.0.weight'] = state['decoder.tick_emb_to_note_emb.0.weight'] * np.float32(3.0)
    score = syn.measure_batch(b, seed=5)
    eps = syn.normal_noise((b, 32), seed=1 if teacher else 2)     # (free-running with seed 1: a 3e-5 top-1 margin in the reference)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 128, dropout, 32, 2, 128, dropout, False, 'folk')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0,
                                capacity=0.0, rand=0, delta=10.0)
    trainer.cuda()
    model.train()
    model.decoder.teacher_forcing_prob = 2.0 if teacher else -1.0
    masks = None
    if dropout > 0:                     # oracle layout (B, T, H); the HIP queues take (T, B, H) uint8
        m_enc, m_beat, m_tick = syn.dropout_masks([(b, 24, 256), (b, 4, 128), (b, 24, 128)], 31, dropout)
        masks = dict(enc=torch.from_numpy(m_enc), beat=torch.from_numpy(m_beat), tick=torch.from_numpy(m_tick))

    def push():
        model.push_noise(torch.from_numpy(eps))
        if masks is not None:
            model.encoder.push_dropout_mask(masks['enc'].transpose(0, 1).contiguous().to(dev))
            model.decoder.push_dropout_masks(masks['beat'].transpose(0, 1).contiguous().to(dev),
                                             masks['tick'].transpose(0, 1).contiguous().to(dev))
    st = torch.from_numpy(score).to(dev)
    trainer.zero_grad()
    push()
    weights, samples, z_dist, _, z, _ = model(st, st, train=True)
    push()
    loss, acc = trainer.loss_and_acc_for_batch((st, st), 0, 0, True)
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()}
    attr = o_attr.attribute_labels(score, *syn.measure_tables())
    ref = o_step.measure_step(state, score, eps, attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, teacher, masks=masks)
    np.testing.assert_array_equal(samples.cpu().numpy(), ref['terms']['samples'])
    close(z, ref['terms']['z'], rtol=0, atol=1e-4)
    close(z_dist.loc, ref['terms']['mu'], rtol=0, atol=1e-4)
    close(weights, ref['terms']['weights'], rtol=1e-4, atol=1e-4)
    terms = {k: v for k, v in trainer.last_terms.items()}
    _compare_step(terms, loss, acc, grads, ref, 3e-3)
    if dropout == 0:                     # the reference itself at this size (dropout off: its masks cannot be injected into nn.GRU)
        g = G(golden_dir, f'measure_step_{"tf" if teacher else "free"}_b256.npz')
        np.testing.assert_array_equal(samples.cpu().numpy(), g['samples'])
        close(attr, g['attr'], rtol=1e-6, atol=1e-7)
        _compare_headline_golden(g, terms, loss, acc, grads, z, z_dist.loc, z_dist.scale)
        w = weights.detach().cpu().numpy()
        close(w[0], g['weights_row0'], rtol=1e-4, atol=1e-4)
        close(w.ravel()[syn.sample_indices('weights', w.size, 128)], g['weights_samp'], rtol=1e-4, atol=1e-4)


def test_free_running_decoder_outside_the_one_launch_kernel(dev):
    """--decoder_hidden_size 32 with a 35-note vocabulary: arvae_tick_free_run is not built for it (vocab > 16*(hidden/16)),
    the decoder must fall back to the tick-by-tick pass and still return the oracle's notes (advisor finding, round 1)."""
    from arvae_amd import ops
    from arvae_amd.measure_vae import MeasureVAE
    from oracle import measure_vae as o_mvae
    assert not ops.tick_free_run_supported(32, 35) and ops.tick_free_run_supported(128, 35) and ops.tick_free_run_supported(32, 32)
    ds = _FolkDataset()
    torch.manual_seed(3)
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.0, 16, 2, 32, 0.0, False, 'folk')
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(3.0)
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.5)
    state = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    model.cuda().eval()
    b = 21
    score = syn.measure_batch(b, seed=77)
    eps = syn.normal_noise((b, 16), seed=78)
    model.push_noise(torch.from_numpy(eps))
    st = torch.from_numpy(score).to(dev)
    with torch.no_grad():
        weights, samples, _, _, z, _ = model(st, st, train=False)
    p = {k: torch.from_numpy(v) for k, v in state.items()}
    w_ref, s_ref, _, _, z_ref = o_mvae.forward(p, torch.from_numpy(score), torch.from_numpy(eps), False)
    np.testing.assert_array_equal(samples.cpu().numpy(), s_ref.numpy())
    close(z, z_ref.numpy(), rtol=0, atol=1e-4)
    close(weights, w_ref.numpy(), rtol=1e-4, atol=1e-4)


def test_epoch_means_under_graph_replay_equal_eager(dev):
    """A multi-batch epoch: the mean loss AND the mean accuracy reported by loss_and_acc_on_epoch are the same whether the
    steps are replayed from HIP graphs or run eagerly (the replayed step's outputs are static buffers the next replay
    overwrites, so the epoch accumulators must start from copies -- advisor finding, round 1), and changing beta
    re-captures (the hyper-parameters are immediates of the captured launches)."""
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    b = 32
    loader = [(x, x) for x in (torch.from_numpy(syn.measure_batch(b, seed=70 + i)).to(dev) for i in range(4))]
    got = {}
    for replay in (True, False):
        ds = _FolkDataset()
        torch.manual_seed(0)
        model = MeasureVAE(ds, 10, 2, 2, 64, 0.0, 16, 2, 64, 0.0, False, 'folk')
        trainer = MeasureVAETrainer(ds, model, lr=1e-3, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0,
                                    capacity=0.0, rand=0, delta=10.0)
        trainer.use_graph_replay = replay
        trainer.use_fused_step = False
        trainer.cuda()
        model.train()
        model.decoder.teacher_forcing_prob = 2.0
        try:
            model.encoder.static_eps = torch.from_numpy(syn.normal_noise((b, 16), seed=3)).to(dev)
            first = trainer.loss_and_acc_on_epoch(loader, epoch_num=0, train=True)
            captured = getattr(trainer, '_graphed', None)
            trainer.beta = 0.5                                  # e.g. an annealing schedule in update_scheduler
            second = trainer.loss_and_acc_on_epoch(loader, epoch_num=1, train=True)
            if replay:
                assert captured is not None and trainer._graphed is not captured
        finally:
            type(model.encoder).static_eps = None
            model.encoder.static_eps = None
        got[replay] = (first, second)
    for (l_a, a_a), (l_b, a_b) in zip(got[True], got[False]):
        close(l_a, l_b, rtol=1e-6)
        close(a_a, a_b, rtol=1e-6)
    assert got[True][1][0] > got[True][0][0]                    # the larger beta shows in the loss


# ---------------------------------------------------------------- row-stream weight gradient (conv32r.hip)
@pytest.mark.parametrize('bias_side', [1, 2])
@pytest.mark.parametrize('lo_size,n', [(16, 1), (16, 2), (16, 7), (16, 130), (16, 512), (8, 1), (8, 3), (8, 37), (8, 512)])
def test_wgrad_row_stream_vs_float64(dev, lo_size, n, bias_side):
    """wgrad32r_kernel (producer / consumer waves over a ring of hi rows) against a float64 conv backward: every batch
    size splits the row stream differently over the workgroups (ranges that start inside an image, a last range that is
    shorter, fewer steps than CUs), and the image borders are zeroed per tap row, so both ends are covered."""
    from arvae_amd import ops
    hi_size = 2 * lo_size
    rs = np.random.RandomState(100 * lo_size + n)
    hi = rs.standard_normal((n, hi_size, hi_size, 32)).astype(np.float32)
    lo = rs.standard_normal((n, lo_size, lo_size, 32)).astype(np.float32)
    link = ops.Link(hi_size, hi_size, 32, lo_size, lo_size, 32, 4, 4, 2, 1)
    dw = torch.zeros(32, 32, 4, 4, device=dev)
    db = torch.zeros(32, device=dev)
    lo_d, hi_d = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)      # kept alive: an operand is a raw pointer
    ops.link_wgrad(link, n, ops._operand(lo_d), ops._operand(hi_d), dw, db, bias_side)
    x = torch.from_numpy(hi).double().permute(0, 3, 1, 2)
    g = torch.from_numpy(lo).double().permute(0, 3, 1, 2)
    w = torch.zeros(32, 32, 4, 4, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=2, padding=1).backward(g)
    want_b = (g if bias_side == 1 else x).sum((0, 2, 3)).numpy()
    err = np.linalg.norm(dw.cpu().numpy().astype(np.float64) - w.grad.numpy()) / np.linalg.norm(w.grad.numpy())
    assert err < 6e-7, err                                   # three-term bf16 split: fp32-level accuracy
    close(db, want_b, rtol=1e-5, atol=1e-5 * float(np.abs(want_b).max()))


# ---------------------------------------------------------------- device RNG (csrc/rng.h) vs oracle/philox.py
def test_philox_draws_vs_oracle(dev):
    """arvae_philox_normal / arvae_philox_keep_mask reproduce the numpy restatement element for element (the uint32 stream
    is pinned by Random123's known-answer vectors in test_oracle_golden.py); moments of a large draw; the stream moves with
    seed, offset and the device step word."""
    import ctypes
    from arvae_amd import _lib, ops
    from oracle import philox
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 100003
    out = torch.empty(n, device=dev)
    seed = 0x123456789abcdef
    assert lib.arvae_philox_normal(ops._ptr(out), n, seed, 7, 2, None, st) == 0
    want = philox.normal(n, seed, offset=7, step=2)
    close(out, want, rtol=2e-5, atol=2e-6)                       # device logf / cosf vs numpy's
    assert abs(float(out.mean())) < 0.02 and abs(float(out.std()) - 1.0) < 0.02
    step = torch.tensor([5], dtype=torch.int32, device=dev)
    out2 = torch.empty(n, device=dev)
    assert lib.arvae_philox_normal(ops._ptr(out2), n, seed, 7, 0, ops._ptr(step), st) == 0
    close(out2, philox.normal(n, seed, offset=7, step=5), rtol=2e-5, atol=2e-6)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    assert lib.arvae_philox_keep_mask(ops._ptr(mask), n, 0.5, seed, 1, 0, None, st) == 0
    np.testing.assert_array_equal(mask.cpu().numpy(), philox.keep_mask(n, 0.5, seed, offset=1))
    assert lib.arvae_philox_keep_mask(ops._ptr(mask), n, 0.75, seed, 2, 0, None, st) == 0
    np.testing.assert_array_equal(mask.cpu().numpy(), philox.keep_mask(n, 0.75, seed, offset=2))
    # several masks of a step as ONE launch (the five Dropout layers of the Morpho-MNIST model): mask j = draw offsets[j], byte
    # for byte the single-mask launch's, ragged lengths included
    try:
        ops.rng_reseed(1234)
        ops.RngState.dev_step = None
        shapes = [(37, 64, 5, 5), (3, 7, 11), (16,), (1024, 8, 19, 19), (5, 64, 22, 22)]
        first = ops.rng_next_offset() + 1
        many = ops.keep_masks(shapes, 0.5, dev)
        for j, (m, shp) in enumerate(zip(many, shapes)):
            assert tuple(m.shape) == shp and m.dtype == torch.uint8
            np.testing.assert_array_equal(m.cpu().numpy().ravel(), philox.keep_mask(int(np.prod(shp)), 0.5, ops.rng_seed(), offset=first + j))
        assert 0.49 < float(many[3].float().mean()) < 0.51
    finally:
        ops.rng_reseed(torch.initial_seed())


def test_device_draws_follow_the_data_parallel_rank(dev):
    """the stream ops.normal_noise / ops.keep_mask draw from is keyed by (torch seed, data-parallel rank): rank 0 = the
    single-process stream, rank 1 = the oracle's Philox under the salted key; a re-seed restarts the draw counter."""
    from arvae_amd import ops
    from oracle import philox
    try:
        draws = {}
        for rank in (0, 1):
            ops.rng_reseed(99)
            ops.RngState.dev_step = None
            ops.rng_set_rank(rank)
            eps = ops.normal_noise((64, 10), dev).cpu().numpy().ravel()
            mask = ops.keep_mask((24, 64, 128), 0.5, dev).cpu().numpy().ravel()
            key = (99 + rank * ops.RANK_SALT) & 0xFFFFFFFFFFFFFFFF
            assert ops.rng_seed() == key and ops.RngState.offset == 2
            close(eps, philox.normal(640, key, offset=0), rtol=2e-5, atol=2e-6)
            np.testing.assert_array_equal(mask, philox.keep_mask(mask.size, 0.5, key, offset=1))
            draws[rank] = (eps, mask)
        assert np.abs(draws[0][0] - draws[1][0]).max() > 0.5
        assert 0.4 < (draws[0][1] != draws[1][1]).mean() < 0.6
    finally:
        ops.rng_set_rank(0)


def test_fused_step_draws_its_own_noise(dev):
    """without pushed noise the fused dSprites step draws eps inside the heads kernel: z = mu + eps * sigma with the eps
    the oracle's Philox gives for (torch seed, this draw's offset), fresh on every step, reproducible under the same seed."""
    from arvae_amd import ops
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    from oracle import philox
    b = 37
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    x, lab = syn.dsprites_batch(b, seed=5)
    runs = []
    for _ in range(2):
        model = DspritesVAE()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        trainer = ImageVAETrainer(DspritesDataset(), model, lr=1e-4, reg_type=('all',), reg_dim=(1, 2, 3, 4, 5), beta=4.0,
                                  gamma=10.0, capacity=0.0, rand=123, delta=1.0)     # torch.manual_seed(123)
        trainer.cuda()
        model.train()
        ops.RngState.offset, ops.RngState.dev_step = 40, None     # (an earlier graph-replay test may have left a device step word)
        zs = []
        for step in range(2):
            trainer.zero_grad()
            loss, _ = trainer.loss_and_acc_for_batch((torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)), 0, step, True)
            loss.backward()
            o = trainer.last_outputs
            eps = ((o['z'] - o['mu']) / o['sigma']).detach().cpu().numpy().ravel()
            close(eps, philox.normal(b * 10, 123, offset=40 + step), rtol=0, atol=2e-3)    # (z - mu) / sigma loses bits
            zs.append(o['z'].detach().clone())
        assert not torch.equal(zs[0], zs[1])
        runs.append(zs)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_debug_checks_raise_like_the_reference(dev, monkeypatch):
    """ARVAE_CHECK=1: a NaN in a weight raises ValueError at the top of the encoder / decoder forward (encoder.py:101-106,
    decoder.py:420-425), a teacher-forced note outside the vocabulary raises from the index check (decoder.py:30-41); off
    by default (no extra launches, no syncs)."""
    from arvae_amd import ops
    from arvae_amd.measure_vae import MeasureVAE
    monkeypatch.setenv('ARVAE_CHECK', '1')
    ds = _FolkDataset()
    torch.manual_seed(1)
    model = MeasureVAE(ds, 10, 2, 2, 64, 0.0, 16, 2, 64, 0.0, False, 'folk')
    model.cuda().eval()
    score = torch.from_numpy(syn.measure_batch(8, seed=3)).to(dev)
    model(score, score, train=False)                         # clean weights, clean indices: passes
    ops.check_finite([torch.ones(5, device=dev)], 'x')
    with pytest.raises(ValueError):
        ops.check_finite([torch.tensor([1.0, float('inf')], device=dev)], 'x')
    with pytest.raises(ValueError):
        ops.check_index(torch.tensor([0, 35], device=dev), 35)
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight[3, 5] = float('nan')
    with pytest.raises(ValueError):
        model(score, score, train=False)
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].weight[3, 5] = 0.0
        model.encoder.lstm.weight_hh_l0[0, 0] = float('nan')
    with pytest.raises(ValueError):
        model(score, score, train=False)
    monkeypatch.setenv('ARVAE_CHECK', '0')
    model(score, score, train=False)                         # checks off: the NaN propagates silently, as without the scan


def test_paired_launches_match_the_separate_launches(dev):
    """A layer's gated data gradient and its weight-gradient partials as ONE grid (conv32.hip pair4_*_kernel, conv_c1.hip
    pair_c1_kernel; dSprites B = 512, where both apply) against ARVAE_NO_PAIR4=1 ARVAE_NO_PAIR_C1=1 (two launches each): the
    halves are the same device functions, so losses and gradients must agree to rounding of the final sums."""
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "from tests.test_hip_parity import run_hip_image_step\n"
        "from arvae_amd import synthetic as syn\n"
        "from oracle import image_vae as o_vae\n"
        "state = syn.synth_state(o_vae.SHAPES['dsprites'], 9, 1.6)\n"
        "x, lab = syn.dsprites_batch(512, seed=5)\n"
        "eps = syn.normal_noise((512, o_vae.Z_DIM['dsprites']), seed=6)\n"
        "got = run_hip_image_step(torch.device('cuda:0'), 'dsprites', state, x, lab, eps, 4.0, 0.0, 'bernoulli', None, train=True)\n"
        "print(json.dumps({'loss': got['loss'], 'gn': {k: float(np.linalg.norm(v)) for k, v in got['grads'].items()},\n"
        "                  'g0': {k: float(np.asarray(v).ravel()[0]) for k, v in got['grads'].items()}}))\n"
        % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    # every horizontal pair of the step against the same work as separate launches: data gradient + weight gradient of the 4x4 /
    # 8x8 and 16x16 / last decoder layers, first layer's weight gradient + Linear weight gradients, weight prep + first conv,
    # regulariser + first decoder conv
    split_env = {k: '1' for k in ('ARVAE_NO_PAIR4', 'ARVAE_NO_PAIR32', 'ARVAE_NO_PAIR_C1', 'ARVAE_NO_PAIR_TAIL', 'ARVAE_NO_PAIR_PREP',
                                  'ARVAE_NO_PAIR_REG')}
    # (the switches exist in the diagnostic build of the library only; 'pair' runs the product library)
    split_env['ARVAE_LIB'] = DIAG_LIB
    for flag, env in (('pair', {}), ('split', split_env)):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    close(res['pair']['loss'], res['split']['loss'], rtol=1e-7)
    for k, v in res['split']['gn'].items():
        close(res['pair']['gn'][k], v, rtol=1e-6, atol=1e-12)
        close(res['pair']['g0'][k], res['split']['g0'][k], rtol=1e-5, atol=1e-9)


def test_chained_forward_layers_match_the_two_launches(dev):
    """conv2 + conv3 of the dSprites encoder as ONE launch (conv32.hip chain_down_kernel: a workgroup runs the 8x8 layer on the
    images whose 16x16 layer it has just stored, its input scale the workgroup's own maximum) against ARVAE_NO_DOWN_CHAIN=1 (two
    launches, the tensor-wide scale): B = 512 and a ragged 500 (runs of whole images in both) chain, B = 64 does not (one tile per
    workgroup) -- the launch labels say which ran; losses and gradients agree to the rounding of a different power-of-two scale."""
    code = (
        "import sys, json, ctypes; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "from tests.test_hip_parity import run_hip_image_step\n"
        "from arvae_amd import synthetic as syn, _lib\n"
        "from oracle import image_vae as o_vae\n"
        "lib = _lib.load()\n"
        "out = {}\n"
        "for b in (512, 500, 64):\n"
        "    state = syn.synth_state(o_vae.SHAPES['dsprites'], 9, 1.6)\n"
        "    x, lab = syn.dsprites_batch(b, seed=5)\n"
        "    eps = syn.normal_noise((b, o_vae.Z_DIM['dsprites']), seed=6)\n"
        "    torch.cuda.synchronize()\n"
        "    lib.arvae_profile_begin(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))\n"
        "    got = run_hip_image_step(torch.device('cuda:0'), 'dsprites', state, x, lab, eps, 4.0, 0.0, 'bernoulli', None, train=True)\n"
        "    buf = ctypes.create_string_buffer(1 << 16)\n"
        "    lib.arvae_profile_end(buf, len(buf))\n"
        "    labels = sorted({ln.split('\\t')[0] for ln in buf.value.decode().splitlines()})\n"
        "    out[str(b)] = {'loss': got['loss'], 'labels': labels, 'gn': {k: float(np.linalg.norm(v)) for k, v in got['grads'].items()}}\n"
        "print(json.dumps(out))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    for flag, env in (('chain', {}), ('two', {'ARVAE_NO_DOWN_CHAIN': '1', 'ARVAE_LIB': DIAG_LIB})):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    label = 'chain(down32<16> + down32<8>)'
    for b in ('512', '500'):
        assert label in res['chain'][b]['labels'] and 'down32_kernel<16>' not in res['chain'][b]['labels']
    assert label not in res['chain']['64']['labels'] and 'down32_kernel<16>' in res['chain']['64']['labels']
    for b in ('512', '500', '64'):
        assert label not in res['two'][b]['labels']
        close(res['chain'][b]['loss'], res['two'][b]['loss'], rtol=1e-6)
        for k, v in res['two'][b]['gn'].items():
            close(res['chain'][b]['gn'][k], v, rtol=1e-5, atol=1e-10)


def test_latent_block_experiment_matches_the_per_layer_path(dev):
    """The latent block (csrc/midblock.hip, the default: the Linear stack + heads + reparameterisation as one launch per pass)
    must give the losses and gradients of the per-layer path (ARVAE_MIDBLOCK=0), dSprites B = 37 and Morpho-MNIST B = 8."""
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "from tests.test_hip_parity import run_hip_image_step\n"
        "from arvae_amd import synthetic as syn\n"
        "from oracle import image_vae as o_vae\n"
        "out = {}\n"
        "for kind, b, gain in (('dsprites', 37, 1.6), ('mnist', 8, 0.7)):\n"
        "    state = syn.synth_state(o_vae.SHAPES[kind], 9, gain)\n"
        "    x, lab = (syn.dsprites_batch if kind == 'dsprites' else syn.mnist_batch)(b, seed=5)\n"
        "    eps = syn.normal_noise((b, o_vae.Z_DIM[kind]), seed=6)\n"
        "    got = run_hip_image_step(torch.device('cuda:0'), kind, state, x, lab, eps, 4.0, 0.0, 'bernoulli', None, train=(kind == 'dsprites'))\n"
        "    out[kind] = {'loss': got['loss'], 'gn': {k: float(np.linalg.norm(v)) for k, v in got['grads'].items()}}\n"
        "print(json.dumps(out))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    # '0': one launch per layer; '1': the latent-block launches (default); 'heads': per layer with ARVAE_HEADS_NEXT=1 (csrc/heads.hip:
    # the decoder's first Linear layer and its data gradient inside the heads kernels, off by default: measured slower)
    # 'rows': the latent block on the row kernels of midblock.hip instead of the clustered ones (midcluster.hip: the default
    # for the dSprites-shaped block); the switches exist in the diagnostic build of the library only, '1' runs the product library
    for flag, env in (('0', {'ARVAE_MIDBLOCK': '0', 'ARVAE_LIB': DIAG_LIB}), ('1', {}),
                      ('rows', {'ARVAE_MID_NO_CLUSTER': '1', 'ARVAE_LIB': DIAG_LIB}),
                      ('heads', {'ARVAE_MIDBLOCK': '0', 'ARVAE_HEADS_NEXT': '1', 'ARVAE_LIB': DIAG_LIB})):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    for flag in ('1', 'rows', 'heads'):
        for kind in ('dsprites', 'mnist'):
            close(res[flag][kind]['loss'], res['0'][kind]['loss'], rtol=1e-6)
            for k, v in res['0'][kind]['gn'].items():
                close(res[flag][kind]['gn'][k], v, rtol=1e-4, atol=1e-9)


def test_latent_block_row_kernel_grows_its_lds_within_one_process(dev):
    """One instantiation of the latent block's row kernels (csrc/midblock.hip) launched with a smaller and then a larger dynamic
    LDS in ONE process: csrc/launch.h keeps the largest size allowed per instantiation and has to raise it for the second model.
    Two Morpho-MNIST-shaped models that differ only in the hidden width, 32 and then 64, whole forward and backward at B = 8.
    mid_describe(): rows per workgroup = 1 for any batch <= the CU count, whatever the width; the 2888-wide layers go to the tile
    GEMMs, so the row pitch is max(hidden, 2 zdim = 32) + 4 floats: 36 and 68, two row buffers each, so
    mid_forward_kernel<1> / mid_backward_kernel<1> ask for 256 bytes more the second time.  32 and 64 are the two smallest widths with different sizes whose wide layers
    stay on the tile GEMMs (their narrow side is a multiple of 32 there).  Each run against the per-layer path (ARVAE_MIDBLOCK=0),
    tolerances of test_latent_block_experiment_matches_the_per_layer_path."""
    code = (
        "import sys, json; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "from collections import OrderedDict\n"
        "from tests.test_hip_parity import MorphoMnistDataset\n"
        "from arvae_amd import synthetic as syn, image_vae as iv\n"
        "from arvae_amd.image_vae_trainer import ImageVAETrainer\n"
        "from oracle import image_vae as o_vae\n"
        "def model_of(width):\n"
        "    m = iv.MnistVAE()\n"
        "    m.enc_lin = iv.LayerStack([(0, iv._dense(2888, width))])\n"
        "    m.enc_mean, m.enc_log_std = iv._dense(width, 16), iv._dense(width, 16)\n"
        "    m.dec_lin = iv.LayerStack([(0, iv._dense(16, width)), (2, iv._dense(width, 2888))])\n"
        "    m.enc_lin_plan = [(0, iv.Link.dense(2888, width, in_perm=(8, 361)))]\n"
        "    m.dec_lin_plan = [(0, iv.Link.dense(16, width)), (2, iv.Link.dense(width, 2888, out_perm=(8, 361)))]\n"
        "    m.head_link = iv.Link.dense(width, 16)\n"
        "    return m\n"
        "out = {}\n"
        "b = 8\n"
        "x, lab = syn.mnist_batch(b, seed=5)\n"
        "eps = syn.normal_noise((b, 16), seed=6)\n"
        "for width in (32, 64):\n"
        "    shapes = OrderedDict((k, tuple(width if d == 256 else d for d in s)) for k, s in o_vae.MNIST_SHAPES.items())\n"
        "    model = model_of(width)\n"
        "    model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.synth_state(shapes, 9, 0.7).items()})\n"
        "    trainer = ImageVAETrainer(MorphoMnistDataset(), model, lr=1e-4, reg_type=('all',), reg_dim=(1, 2, 3, 4, 5, 6), dec_dist='bernoulli',\n"
        "                              beta=4.0, gamma=10.0, capacity=0.0, rand=0, delta=1.0)\n"
        "    trainer.cuda()\n"
        "    model.eval()\n"
        "    model.push_noise(torch.from_numpy(eps))\n"
        "    trainer.zero_grad()\n"
        "    loss, acc = trainer.loss_and_acc_for_batch((torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()), 0, 0, False)\n"
        "    loss.backward()\n"
        "    out[str(width)] = {'loss': float(loss), 'gn': {k: float(np.linalg.norm(p.grad.detach().cpu().numpy())) for k, p in model.named_parameters()}}\n"
        "print(json.dumps(out))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    for flag, env in (('0', {'ARVAE_MIDBLOCK': '0', 'ARVAE_LIB': DIAG_LIB}), ('1', {})):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    for width in ('32', '64'):
        close(res['1'][width]['loss'], res['0'][width]['loss'], rtol=1e-6)
        for k, v in res['0'][width]['gn'].items():
            close(res['1'][width]['gn'][k], v, rtol=1e-4, atol=1e-9)


# ---------------------------------------------------------------- the epoch loop itself (Trainer.train_model) vs the oracle's trajectory
def _close_after_adam(got, want, steps):
    """weights after `steps` Adam updates (lr 1e-4): atol 1e-5 for all but a handful of entries.  Adam moves an entry by up
    to lr per step whatever the gradient's size, so an entry whose gradient is ~0 turns a last-bit gradient difference into
    a visible step: at most 1e-3 of the entries may exceed 1e-5 (37 of 131 072 did in one tensor with another exact split of
    the conv operands), none may be off by more than half a step per update."""
    d = np.abs(np.asarray(got.detach().cpu() if hasattr(got, 'detach') else got, np.float64) - np.asarray(want, np.float64))
    assert d.max() <= 0.5e-4 * steps, d.max()
    assert (d > 1e-5).mean() <= 1e-3, ((d > 1e-5).sum(), d.size)


class _ListLoaders:
    """a dataset whose data_loaders() hands out fixed lists of batches (train, validation, test)"""

    def __init__(self, train, val):
        self.train, self.val = train, val

    def data_loaders(self, batch_size, split=(0.70, 0.20), **_):
        return self.train, self.val, self.val


def test_image_train_model_two_epochs_track_the_oracle(dev, tmp_path, monkeypatch):
    """utils/trainer.py:39-154 through the build's own epoch loop: train_model for 2 epochs x 3 batches (+ one validation
    batch per epoch, which must not move the weights) ends on the weights of the oracle's six chained steps (atol 1e-5),
    and the per-epoch mean training loss it computes on the device is the mean of the oracle's step losses."""
    from arvae_amd.image_vae import DspritesVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path))

    class DspritesDataset(_ListLoaders):
        pass
    b = 16
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 5, 1.6)
    train = [syn.dsprites_batch(b, seed=300 + i) for i in range(3)]
    val = [syn.dsprites_batch(b, seed=310)]
    eps_t = [syn.normal_noise((b, 10), seed=320 + i) for i in range(6)]
    eps_v = [syn.normal_noise((b, 10), seed=330 + i) for i in range(2)]
    to_t = lambda xs: [(torch.from_numpy(x), torch.from_numpy(lab)) for x, lab in xs]
    model = DspritesVAE()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = ImageVAETrainer(DspritesDataset(to_t(train), to_t(val)), model, lr=1e-4, reg_type=('all',),
                              reg_dim=(1, 2, 3, 4, 5), beta=4.0, gamma=10.0, capacity=0.0, rand=0, delta=1.0)
    trainer.cuda()
    for epoch in range(2):                      # the order the loop draws: three training steps, then the validation batch
        for e in eps_t[3 * epoch:3 * epoch + 3] + [eps_v[epoch]]:
            model.push_noise(torch.from_numpy(e))
    means = []
    keep = trainer.print_epoch_stats
    trainer.print_epoch_stats = lambda *a: (means.append(a[2:]), keep(*a))[1]
    trainer.train_model(batch_size=b, num_epochs=2, log=False)
    assert not model._eps_queue and os.path.exists(model.filepath)
    cur, adam, losses_ref = state, None, []
    for k in range(6):
        x, lab = train[k % 3]
        ref = o_step.image_step('dsprites', cur, x, lab, eps_t[k], (1, 2, 3, 4, 5), 4.0, 10.0, 1.0, adam_state=adam,
                                step_no=k + 1)
        cur, adam = ref['params'], ref['adam']
        losses_ref.append(ref['terms']['loss'])
    for name, p in model.named_parameters():
        _close_after_adam(p, cur[name], 6)
    assert len(means) == 2
    for epoch in range(2):
        close(means[epoch][0], np.mean(losses_ref[3 * epoch:3 * epoch + 3]), rtol=1e-4)
    # the validation pass used the weights after the epoch's last step and did not touch them
    ref_val = o_step.image_step('dsprites', cur, *val[0], eps_v[1], (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)
    close(means[1][2], ref_val['terms']['loss'], rtol=1e-4)
    saved = torch.load(model.filepath, map_location='cpu')
    for name in state:
        _close_after_adam(saved[name], cur[name], 6)


@pytest.mark.parametrize('replay', [False, True], ids=['eager', 'graph_replay'])
def test_measure_train_model_two_epochs_track_the_oracle(dev, tmp_path, monkeypatch, replay):
    """the same for MeasureVAETrainer, whose epoch loop replays its steps from HIP graphs by default: 2 epochs x 3 batches,
    eager and replayed, against the oracle's six chained steps (teacher-forced, no dropout; the noise of step k reaches
    the captured graph through a device buffer the loader refreshes before handing out batch k)."""
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    from oracle import attributes as o_attr
    from oracle import measure_vae as o_mvae
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path))
    b = 32
    state = syn.synth_state(o_mvae.shapes(), 4)
    scores = [syn.measure_batch(b, seed=400 + i) for i in range(3)]
    val = syn.measure_batch(b, seed=410)
    eps_t = [syn.normal_noise((b, 32), seed=420 + i) for i in range(6)]
    static = torch.zeros(b, 32, device=dev)

    class _Loader:
        """hands out the batches and, just before each, moves that step's noise into the static device buffer"""

        def __init__(self, batches, noise, counter):
            self.batches, self.noise, self.counter = batches, noise, counter

        def __len__(self):
            return len(self.batches)

        def __iter__(self):
            for s in self.batches:
                if self.noise is not None:
                    static.copy_(torch.from_numpy(self.noise[self.counter[0]]))
                    self.counter[0] += 1
                yield torch.from_numpy(s), torch.from_numpy(s)

    class FolkData(_FolkDataset):
        def data_loaders(self, batch_size, split=(0.70, 0.20), **_):
            return self.loaders

    ds = FolkData()
    counter = [0]
    ds.loaders = (_Loader(scores, eps_t, counter), _Loader([val], None, counter), None)
    model = MeasureVAE(ds, 10, 2, 2, 128, 0.0, 32, 2, 128, 0.0, False, 'folk')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0,
                                capacity=0.0, rand=0, delta=10.0)
    trainer.use_graph_replay = replay
    trainer.use_fused_step = not replay       # replayed: the per-layer path from HIP graphs; eager: the whole-model executor
    trainer.cuda()
    model.decoder.teacher_forcing_prob = 2.0
    means = []
    keep = trainer.print_epoch_stats
    trainer.print_epoch_stats = lambda *a: (means.append(a[2:]), keep(*a))[1]
    try:
        model.encoder.static_eps = static
        trainer.train_model(batch_size=b, num_epochs=2, log=False)
    finally:
        type(model.encoder).static_eps = None
        model.encoder.static_eps = None
    assert counter[0] == 6
    if replay:
        assert getattr(trainer, '_graphed', None) is not None and trainer.use_graph_replay, 'the steps were not replayed'
    cur, adam, losses_ref = state, None, []
    tables = syn.measure_tables()
    for k in range(6):
        sc = scores[k % 3]
        attr = o_attr.attribute_labels(sc, *tables)
        ref = o_step.measure_step(cur, sc, eps_t[k], attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, True, adam_state=adam,
                                  step_no=k + 1)
        cur, adam = ref['params'], ref['adam']
        losses_ref.append(ref['terms']['loss'])
    for name, p in model.named_parameters():
        _close_after_adam(p, cur[name], 6)
    for epoch in range(2):
        close(means[epoch][0], np.mean(losses_ref[3 * epoch:3 * epoch + 3]), rtol=1e-4)


# ---------------------------------------------------------------- what the 2e-3 gradient tolerance hides: an error budget in float64
def test_gradient_error_budget_vs_float64(dev):
    """The step tests above allow whole-tensor relative L2 2e-3 against the fp32 CPU oracle, because a ReLU whose
    pre-activation is ~0 may land on the other side in another fp32 summation order.  This test measures instead of assuming:
    the oracle's own step is run in float64 and in float32 on the same tensors, and per gradient tensor the HIP path's
    distance to the float64 result must stay within 2x the fp32 CPU path's distance to it (+ a 2e-6 floor for tensors the
    CPU happens to get almost exactly).  A flipped unit is a rare event of ONE run (about 0.1 expected per step at this size:
    it moved one tensor by 5e-5 in one of the runs this test has seen), a kernel error is there every time: three runs on
    different inputs, and every tensor must meet the budget in at least two of them."""
    b = 64
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    st64 = {k: v.astype(np.float64) for k, v in state.items()}
    ok = {name: 0 for name in state}
    worst = 0.0
    for run in range(3):
        x, lab = syn.dsprites_batch(b, seed=1234 + run)
        eps = syn.normal_noise((b, 10), seed=12 + run)
        got = run_hip_image_step(dev, 'dsprites', state, x, lab, eps, 4.0, 0.0, 'bernoulli', None)
        ref32 = o_step.image_step('dsprites', state, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)
        ref64 = o_step.image_step('dsprites', st64, x.astype(np.float64), lab.astype(np.float64), eps.astype(np.float64),
                                  (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)
        for name in state:
            want = ref64['grads'][name].ravel()
            scale = np.linalg.norm(want) + 1e-30
            e_hip = np.linalg.norm(got['grads'][name].astype(np.float64).ravel() - want) / scale
            e_cpu = np.linalg.norm(ref32['grads'][name].astype(np.float64).ravel() - want) / scale
            if e_hip <= 2.0 * e_cpu + 2e-6:
                ok[name] += 1
                worst = max(worst, e_hip / max(e_cpu, 1e-12))
        for k in ('recons', 'dist', 'reg', 'loss'):
            close(got['loss'] if k == 'loss' else got['terms'][k], ref64['terms'][k], rtol=1e-5)
    assert all(v >= 2 for v in ok.values()), {k: v for k, v in ok.items() if v < 2}
    print(f'worst HIP / fp32-CPU error ratio vs float64 among the runs within budget: {worst:.2f}; runs within budget per tensor: '
          f'{min(ok.values())}..{max(ok.values())} of 3')


def test_adam_clears_the_gradient_arena_and_zero_grad_knows(dev):
    """FlatAdam.step() clears the gradient arena in the kernel that consumes it, so the zero_grad() of the next step
    launches nothing -- unless a backward pass ran in between (fused executor: mark_dirty; torch's own accumulation: the
    post-accumulate hooks), and never while a step is being captured.  The update itself is the plain kernel's."""
    from arvae_amd.optim import FlatAdam
    torch.manual_seed(0)
    results = []
    for zero_in_step in (True, False):
        params = [torch.nn.Parameter(torch.linspace(-1, 1, n, device=dev).clone()) for n in (37, 1024, 5)]
        opt = FlatAdam(params, lr=1e-3, zero_grads_in_step=zero_in_step)
        for step in range(3):
            opt.zero_grad()
            assert float(opt.grad_arena.abs().max()) == 0.0
            loss = sum((p * p).sum() * (i + 1) for i, p in enumerate(params))
            loss.backward()                                  # torch accumulates into the arena views: hooks mark it dirty
            assert not opt._arena_clean and float(opt.grad_arena.abs().max()) > 0.0
            opt.step()
            assert opt._arena_clean == zero_in_step
            assert (float(opt.grad_arena.abs().max()) == 0.0) == zero_in_step
        results.append(torch.cat([p.detach().reshape(-1) for p in params]).clone())
        # a backward pass between step() and zero_grad(): the arena is dirty again and zero_grad() must clear it
        loss = sum((p * p).sum() for p in params)
        loss.backward()
        assert not opt._arena_clean
        opt.zero_grad()
        assert float(opt.grad_arena.abs().max()) == 0.0
    assert torch.equal(results[0], results[1])

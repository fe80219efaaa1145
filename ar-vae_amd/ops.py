"""torch.autograd wrappers over the libarvae_hip.so C-ABI (PyTorch = bookkeeping only).

Every op takes fp32 contiguous HIP tensors and launches hand-written gfx950
kernels on the current stream.  There is no CPU path: CPU tensors raise.

Activation tensors are channels-last ([N, H, W, C]; [B, F] for dense layers).
"""
import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import LinkDesc, OperandDesc

ACT_NONE, ACT_RELU, ACT_SELU = 0, 1, 2
RECON_DIST = {'bernoulli': 0, 'gaussian': 1}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('arvae_amd ops run on the GPU only (HIP kernels, no CPU fallback); '
                               'got a CPU tensor -- call .cuda() on the model/inputs')
        if t.dtype not in (torch.float32, torch.uint8, torch.int64):
            raise TypeError(f'unsupported dtype {t.dtype}')
        if not t.is_contiguous():
            raise ValueError('arvae_amd ops need contiguous tensors')


def _operand(v, y=None, mask=None, act=ACT_NONE):
    return OperandDesc(_ptr(v), _ptr(y), _ptr(mask), act)


@dataclass(frozen=True)
class Link:
    """Static geometry of a strided link (see include/arvae_hip.h): hi [.,hh,hw,chi] <-> lo [.,lh,lw,clo]."""
    hh: int
    hw: int
    chi: int
    lh: int
    lw: int
    clo: int
    kh: int = 1
    kw: int = 1
    stride: int = 1
    pad: int = 0
    hi_perm: Tuple[int, int] = (0, 0)
    lo_perm: Tuple[int, int] = (0, 0)

    def desc(self, n):
        return LinkDesc(n, self.hh, self.hw, self.chi, self.lh, self.lw, self.clo, self.kh, self.kw, self.stride,
                        self.pad, self.hi_perm[0], self.hi_perm[1], self.lo_perm[0], self.lo_perm[1])

    @staticmethod
    def dense(in_features, out_features, in_perm=(0, 0), out_perm=(0, 0)):
        return Link(1, 1, in_features, 1, 1, out_features, hi_perm=in_perm, lo_perm=out_perm)

    def hi_shape(self, n):
        return (n, self.chi) if self.hh == self.hw == self.lh == self.lw == 1 else (n, self.hh, self.hw, self.chi)

    def lo_shape(self, n):
        return (n, self.clo) if self.hh == self.hw == self.lh == self.lw == 1 else (n, self.lh, self.lw, self.clo)


# ------------------------------------------------------------------------------------------------
# per-kernel timing hook (bench.py): HIP events on the launch stream around every library call
# ------------------------------------------------------------------------------------------------
_PROFILE = None


def profile_begin():
    global _PROFILE
    _PROFILE = []


def profile_end():
    """-> {kernel family: dict(calls, ms, flop, bytes)} aggregated over the recorded launches."""
    global _PROFILE
    rec, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    out = {}
    for name, flop, nbytes, e0, e1 in rec or []:
        d = out.setdefault(name, dict(calls=0, ms=0.0, flop=0.0, bytes=0.0))
        d['calls'] += 1
        d['ms'] += e0.elapsed_time(e1)
        d['flop'] += flop
        d['bytes'] += nbytes
    return out


class _timed:
    def __init__(self, name, flop=0.0, nbytes=0.0):
        self.args = (name, flop, nbytes)

    def __enter__(self):
        if _PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _PROFILE is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _PROFILE.append(self.args + (self.e0, e1))


def _link_cost(link, n, op):
    """(algorithmic FLOP, layer-boundary bytes) of one link launch."""
    macs = n * link.lh * link.lw * link.clo * link.chi * link.kh * link.kw
    hi_b, lo_b = 4 * n * link.hh * link.hw * link.chi, 4 * n * link.lh * link.lw * link.clo
    wt_b = 4 * link.clo * link.chi * link.kh * link.kw
    return 2.0 * macs, float(hi_b + lo_b + wt_b)


# ------------------------------------------------------------------------------------------------
# raw launches (no autograd)
# ------------------------------------------------------------------------------------------------
def _link_ws(lib, desc, device):
    """the caller-owned scratch arvae_link_down / _up ask for (most links: none)"""
    n = lib.arvae_link_ws_floats(ctypes.byref(desc))
    return torch.empty(n, device=device, dtype=torch.float32) if n else None


def link_down(link: Link, n, hi_op, wt, bias, act, out_mask, out=None):
    lib = _lib.load()
    lo = out if out is not None else torch.empty(link.lo_shape(n), device=wt.device, dtype=torch.float32)
    d = link.desc(n)
    ws = _link_ws(lib, d, wt.device)
    with _timed('link_gemm<down>', *_link_cost(link, n, hi_op)):
        _lib.check(lib.arvae_link_down(ctypes.byref(d), ctypes.byref(hi_op), _ptr(wt), _ptr(bias), act,
                                       _ptr(out_mask), _ptr(lo), _ptr(ws), _stream()), 'link_down')
    return lo


def link_up(link: Link, n, lo_op, wt, bias, act, out_mask, out=None):
    lib = _lib.load()
    hi = out if out is not None else torch.empty(link.hi_shape(n), device=wt.device, dtype=torch.float32)
    d = link.desc(n)
    name = 'up_single_channel' if (link.chi == 1 and not lo_op.y) else 'link_gemm<up>'
    ws = _link_ws(lib, d, wt.device)
    with _timed(name, *_link_cost(link, n, lo_op)):
        _lib.check(lib.arvae_link_up(ctypes.byref(d), ctypes.byref(lo_op), _ptr(wt), _ptr(bias), act,
                                     _ptr(out_mask), _ptr(hi), _ptr(ws), _stream()), 'link_up')
    return hi


def link_wgrad(link: Link, n, lo_op, hi_op, dwt, dbias=None, bias_side=0):
    """dwt += weight gradient; dbias += bias gradient (bias_side 1: sums of lo, 2: sums of hi). Accumulates."""
    lib = _lib.load()
    d = link.desc(n)
    nws = lib.arvae_link_wgrad_ws_floats(ctypes.byref(d))
    ws = torch.empty(nws, device=dwt.device, dtype=torch.float32) if nws else None
    with _timed('link_wgrad', *_link_cost(link, n, lo_op)):
        _lib.check(lib.arvae_link_wgrad(ctypes.byref(d), ctypes.byref(lo_op), ctypes.byref(hi_op), _ptr(dwt),
                                        _ptr(dbias), bias_side if dbias is not None else 0, _ptr(ws), _stream()),
                   'link_wgrad')
    return dwt


def channel_sum(op, rows, channels, perm, out):
    """out += per-channel sums (accumulates)."""
    lib = _lib.load()
    ws = torch.empty(lib.arvae_channel_sum_ws_floats(rows, channels), device=out.device, dtype=torch.float32)
    with _timed('channel_sum', float(rows * channels), 4.0 * rows * channels * (2 if op.y else 1)):
        _lib.check(lib.arvae_channel_sum(ctypes.byref(op), rows, channels, perm[0], perm[1], _ptr(out), _ptr(ws),
                                         _stream()), 'channel_sum')
    return out


def wide_dense(link: Link, n, mode, w, x=None, g=None, bias=None, dw=None, dbias=None):
    """One product of a wide Linear layer on the latent block's three-term bf16 tile kernels (csrc/dense.hip wide_gemm_x3_kernel /
    wide_wgrad_x3_kernel), outside the whole-model executor.  mode 0: x W^T (+ bias), 1: g W, 2: dw += g^T x, dbias += sums of g."""
    lib = _lib.load()
    d = link.desc(n)
    ws = torch.empty(lib.arvae_wide_dense_ws_floats(ctypes.byref(d)), device=w.device, dtype=torch.float32)
    out = None if mode == 2 else torch.empty((n, link.clo if mode == 0 else link.chi), device=w.device, dtype=torch.float32)
    with _timed('wide_dense', 2.0 * n * link.chi * link.clo, 0.0):
        _lib.check(lib.arvae_wide_dense(ctypes.byref(d), mode, _ptr(x), _ptr(g), _ptr(w), _ptr(bias), _ptr(out), _ptr(dw), _ptr(dbias),
                                        _ptr(ws), _stream()), 'wide_dense')
    return dw if mode == 2 else out


LONG_BATCH_ROWS = 2048      # csrc/dense.h DENSE_SPLIT_MIN_ROWS: Linear layers over this many rows run on the rows-GEMM kernels


def _plain_gradient(g, y, mask, act, link, n):
    """operand of a Linear layer's output gradient; for long batches with an activation / mask to fold in, the folded
    gradient is written out once so that both the data- and the weight-gradient run on the plain-operand kernels."""
    dense_long = n >= LONG_BATCH_ROWS and link.hh == link.hw == link.lh == link.lw == 1
    # the wide stride-1 convolution kernels (csrc/conv64.hip) gather their operands once per tap
    wide_conv = link.stride == 1 and link.kh * link.kw > 1 and (link.chi % 32 == 0 or link.clo % 32 == 0)
    if (act != ACT_NONE or mask is not None) and (dense_long or wide_conv):
        lib = _lib.load()
        out = torch.empty_like(g)
        op = _operand(g, y, mask, act)
        _lib.check(lib.arvae_operand_apply(ctypes.byref(op), g.numel(), _ptr(out), _stream()), 'operand_apply')
        return _operand(out), out
    if act == ACT_NONE and mask is None:
        return _operand(g), g
    return _operand(g, y, mask, act), g


# ------------------------------------------------------------------------------------------------
# batch-sized Linear weight gradients of one backward pass, launched together when the pass ends
# ------------------------------------------------------------------------------------------------
_WGRAD_QUEUE = []
DEFER_DENSE_WGRADS = True


def _flush_dense_wgrads():
    """one launch for every queued Linear weight gradient (csrc/dense.hip dense_wgrad_batch_kernel)."""
    global _WGRAD_QUEUE
    if not _WGRAD_QUEUE:
        return
    queue, _WGRAD_QUEUE = _WGRAD_QUEUE, []
    lib = _lib.load()
    jobs = (_lib.DenseWgradJob * len(queue))()
    for j, (gop, x, dw, db, rows, n_in, n_out, _keep) in zip(jobs, queue):
        j.g, j.x, j.dw, j.dbias = gop, _ptr(x), _ptr(dw), _ptr(db)
        j.rows, j.n_in, j.n_out = rows, n_in, n_out
    with _timed('dense_wgrad_batch', 0.0, 0.0):
        _lib.check(lib.arvae_dense_wgrad_batch(jobs, len(queue), _stream()), 'dense_wgrad_batch')


def _defer_dense_wgrad(link, n, gop, keep, x, dw, db):
    """queue dw += g^T x (db += colsum g) until the running backward pass ends; False if it cannot be queued."""
    if not DEFER_DENSE_WGRADS or n >= LONG_BATCH_ROWS or link.hi_perm[0] or link.lo_perm[0]:
        return False
    if not (link.hh == link.hw == link.lh == link.lw == link.kh == link.kw == 1):
        return False
    if any(q[2].data_ptr() == dw.data_ptr() for q in _WGRAD_QUEUE):
        return False          # two jobs of one launch must not add into the same tensor (a weight used at several steps)
    if not _WGRAD_QUEUE:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_flush_dense_wgrads)
        except RuntimeError:                                  # not inside a backward pass
            return False
    _WGRAD_QUEUE.append((gop, x, dw, db, n, link.chi, link.clo, keep))
    return True


# bumped by every gradient the kernels add straight into a parameter's `.grad` buffer (autograd gets None back, so the
# optimizer's post-accumulate hooks do not fire): FlatAdam compares it with the value it saw at its last step()
GRAD_WRITE_EPOCH = [0]


def _grad_target(param):
    """Where a parameter gradient is accumulated.  When the parameter already owns a `.grad` buffer (the
    trainer's flat gradient arena after zero_grad()), the kernels add straight into it and autograd gets
    None back -- no zero-fill and no AccumulateGrad add per tensor.  Otherwise a fresh zeroed tensor is
    returned through autograd as usual."""
    g = param.grad
    if g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.device == param.device:
        GRAD_WRITE_EPOCH[0] += 1          # no AccumulateGrad (hence no hook) will run for this write: optim.FlatAdam looks here
        return g, True
    return torch.zeros_like(param), False


# ------------------------------------------------------------------------------------------------
# layers
# ------------------------------------------------------------------------------------------------
class _LinkDownFn(Function):
    """nn.Conv2d / nn.Linear forward (+bias, activation, dropout keep-mask) and its backward."""

    @staticmethod
    def forward(ctx, hi, wt, bias, link, act, mask):
        _dev(hi, wt, bias, mask)
        n = hi.shape[0]
        lo = link_down(link, n, _operand(hi), wt, bias, act, mask)
        ctx.link, ctx.act, ctx.n = link, act, n
        ctx.save_for_backward(hi, wt, lo, mask)
        ctx.wt_ref, ctx.bias_ref = wt, bias
        return lo

    @staticmethod
    @once_differentiable
    def backward(ctx, g_lo):
        hi, wt, lo, mask = ctx.saved_tensors
        link, n = ctx.link, ctx.n
        g_lo = g_lo.contiguous()
        gop, _keep = _plain_gradient(g_lo, lo, mask, ctx.act, link, n)
        d_hi = d_wt = d_bias = None
        if ctx.needs_input_grad[0]:
            d_hi = link_up(link, n, gop, wt, None, ACT_NONE, None)
        want_bias = ctx.bias_ref is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            buf, direct = _grad_target(ctx.wt_ref)
            bbuf, bdirect = _grad_target(ctx.bias_ref) if want_bias else (None, True)
            # queued launches add into the parameters' own .grad buffers; a gradient handed back through autograd
            # must be complete when backward() returns it, so those go out immediately
            if not (direct and bdirect and _defer_dense_wgrad(link, n, gop, (g_lo, _keep, lo, mask, hi), hi, buf, bbuf)):
                link_wgrad(link, n, gop, _operand(hi), buf, bbuf, 1)
            d_wt = None if direct else buf
            d_bias = None if bdirect else bbuf
        elif want_bias:
            bbuf, bdirect = _grad_target(ctx.bias_ref)
            channel_sum(gop, n * link.lh * link.lw, link.clo, link.lo_perm, bbuf)
            d_bias = None if bdirect else bbuf
        return d_hi, d_wt, d_bias, None, None, None


class _LinkUpFn(Function):
    """nn.ConvTranspose2d forward (+bias, activation, dropout keep-mask) and its backward."""

    @staticmethod
    def forward(ctx, lo, wt, bias, link, act, mask):
        _dev(lo, wt, bias, mask)
        n = lo.shape[0]
        hi = link_up(link, n, _operand(lo), wt, bias, act, mask)
        ctx.link, ctx.act, ctx.n = link, act, n
        ctx.save_for_backward(lo, wt, hi, mask)
        ctx.wt_ref, ctx.bias_ref = wt, bias
        return hi

    @staticmethod
    @once_differentiable
    def backward(ctx, g_hi):
        lo, wt, hi, mask = ctx.saved_tensors
        link, n = ctx.link, ctx.n
        g_hi = g_hi.contiguous()
        gop, _keep = _plain_gradient(g_hi, hi, mask, ctx.act, link, n)
        d_lo = d_wt = d_bias = None
        if ctx.needs_input_grad[0]:
            d_lo = link_down(link, n, gop, wt, None, ACT_NONE, None)
        want_bias = ctx.bias_ref is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            buf, direct = _grad_target(ctx.wt_ref)
            bbuf, bdirect = _grad_target(ctx.bias_ref) if want_bias else (None, True)
            link_wgrad(link, n, _operand(lo), gop, buf, bbuf, 2)
            d_wt = None if direct else buf
            d_bias = None if bdirect else bbuf
        elif want_bias:
            bbuf, bdirect = _grad_target(ctx.bias_ref)
            channel_sum(gop, n * link.hh * link.hw, link.chi, link.hi_perm, bbuf)
            d_bias = None if bdirect else bbuf
        return d_lo, d_wt, d_bias, None, None, None


def conv_down(hi, wt, bias, link, act=ACT_NONE, mask=None):
    return _LinkDownFn.apply(hi, wt, bias, link, act, mask)


def conv_up(lo, wt, bias, link, act=ACT_NONE, mask=None):
    return _LinkUpFn.apply(lo, wt, bias, link, act, mask)


def dense(x, wt, bias, link, act=ACT_NONE):
    return _LinkDownFn.apply(x, wt, bias, link, act, None)


# ------------------------------------------------------------------------------------------------
# latent head / KL
# ------------------------------------------------------------------------------------------------
class _LatentFn(Function):
    @staticmethod
    def forward(ctx, mu, log_std, eps):
        _dev(mu, log_std, eps)
        lib = _lib.load()
        sigma, z = torch.empty_like(mu), torch.empty_like(mu)
        _lib.check(lib.arvae_latent_fwd(_ptr(mu), _ptr(log_std), _ptr(eps), mu.numel(), _ptr(sigma), _ptr(z),
                                        _stream()), 'latent_fwd')
        ctx.save_for_backward(eps, sigma)
        return sigma, z

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sigma, g_z):
        eps, sigma = ctx.saved_tensors
        lib = _lib.load()
        g_sigma = None if g_sigma is None else g_sigma.contiguous()
        g_z = None if g_z is None else g_z.contiguous()
        d_mu, d_ls = torch.empty_like(sigma), torch.empty_like(sigma)
        _lib.check(lib.arvae_latent_bwd(_ptr(g_z), _ptr(g_sigma), _ptr(eps), _ptr(sigma), sigma.numel(), _ptr(d_mu),
                                        _ptr(d_ls), _stream()), 'latent_bwd')
        return d_mu, d_ls, None


def latent_head(mu, log_std, eps):
    """-> (sigma, z) with sigma = exp(log_std), z = mu + eps * sigma."""
    return _LatentFn.apply(mu.contiguous(), log_std.contiguous(), eps.contiguous())


class _KLDFn(Function):
    @staticmethod
    def forward(ctx, mu, sigma, prior_mu, prior_sigma, beta, capacity):
        _dev(mu, sigma, prior_mu, prior_sigma, capacity)
        lib = _lib.load()
        b, zd = mu.shape
        out = torch.empty(2, device=mu.device, dtype=torch.float32)
        _lib.check(lib.arvae_kld_fwd(_ptr(mu), _ptr(sigma), _ptr(prior_mu), _ptr(prior_sigma), b, zd, beta,
                                     _ptr(capacity), _ptr(out), _stream()), 'kld_fwd')
        ctx.beta = beta
        ctx.save_for_backward(mu, sigma, prior_mu, prior_sigma, out, capacity)
        return out[0:1] if capacity is not None else out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, sigma, prior_mu, prior_sigma, out, capacity = ctx.saved_tensors
        lib = _lib.load()
        b, zd = mu.shape
        g = g.reshape(1).contiguous()
        d_mu, d_sigma = torch.empty_like(mu), torch.empty_like(mu)
        _lib.check(lib.arvae_kld_bwd(_ptr(g), _ptr(mu), _ptr(sigma), _ptr(prior_mu), _ptr(prior_sigma), b, zd,
                                     ctx.beta, _ptr(out), _ptr(capacity), _ptr(d_mu), _ptr(d_sigma), _stream()),
                   'kld_bwd')
        return d_mu, d_sigma, None, None, None, None


def kld_loss(mu, sigma, beta, capacity=None, prior_mu=None, prior_sigma=None):
    """beta * |mean_b sum_z KL(N(mu,sigma) || prior) - c|; prior None = N(0,1).
    capacity: 1-element tensor (result has shape (1,), like the reference) or None."""
    if capacity is not None:
        capacity = capacity.reshape(1).to(torch.float32).contiguous()
    return _KLDFn.apply(mu.contiguous(), sigma.contiguous(), prior_mu, prior_sigma, float(beta), capacity)


# ------------------------------------------------------------------------------------------------
# attribute regularisation
# ------------------------------------------------------------------------------------------------
class _RegLossFn(Function):
    @staticmethod
    def forward(ctx, z, labels, dims, gamma, delta, z_cols, lab_cols):
        _dev(z, labels, z_cols, lab_cols)
        lib = _lib.load()
        n_rows, ldz = z.shape
        ldl = labels.shape[1]
        zc = z if z_cols is None else z_cols
        lc = labels if lab_cols is None else lab_cols
        if zc.shape[1] != ldz or lc.shape[1] != ldl or zc.shape[0] != lc.shape[0]:
            raise ValueError('column tensors must have the row tensors\' widths')
        r = len(dims)
        ws = torch.empty(lib.arvae_reg_loss_ws_floats(n_rows, r), device=z.device, dtype=torch.float32)
        loss = torch.empty((), device=z.device, dtype=torch.float32)
        dz = torch.empty_like(z)
        cdims = (ctypes.c_int32 * r)(*dims)
        with _timed('reg_loss', 0.0, 8.0 * (n_rows + zc.shape[0]) * r):
            _lib.check(lib.arvae_reg_loss(_ptr(z), _ptr(labels), n_rows, _ptr(zc), _ptr(lc), zc.shape[0], ldz, ldl,
                                          cdims, r, gamma, delta, _ptr(ws), _ptr(loss), _ptr(dz), _stream()),
                       'reg_loss')
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return scale_by_scalar(g, dz), None, None, None, None, None, None


def reg_loss(z, labels, dims, gamma, delta, z_cols=None, lab_cols=None):
    """sum over dims of gamma * mean_ij |tanh(delta (z_i - z_j)) - sign(a_i - a_j)|, all dims in one launch.
    z[:, d] pairs with labels[:, d].  z_cols/lab_cols: the all-gathered global batch under data parallelism
    (rows = this rank's samples); the mean is then over len(cols)^2 pairs."""
    dims = tuple(int(d) for d in dims)
    if len(dims) == 0:
        raise ValueError('reg_loss needs at least one dimension')
    if len(set(dims)) != len(dims):
        raise ValueError(f'reg_loss: a dimension is listed twice in {dims} (dz has one entry per column)')
    return _RegLossFn.apply(z.contiguous(), labels.contiguous().to(torch.float32), dims, float(gamma), float(delta),
                            None if z_cols is None else z_cols.contiguous(),
                            None if lab_cols is None else lab_cols.contiguous().to(torch.float32))


def scale_by_scalar(g, x):
    lib = _lib.load()
    g = g.reshape(1).contiguous()
    y = torch.empty_like(x)
    _lib.check(lib.arvae_scale_by_scalar(_ptr(g), _ptr(x), x.numel(), _ptr(y), _stream()), 'scale_by_scalar')
    return y


# ------------------------------------------------------------------------------------------------
# reconstruction terms
# ------------------------------------------------------------------------------------------------
class _ImageReconFn(Function):
    @staticmethod
    def forward(ctx, logits, x, dist):
        _dev(logits, x)
        lib = _lib.load()
        count, batch = logits.numel(), logits.shape[0]
        ws = torch.empty(lib.arvae_recon_ws_floats(count), device=x.device, dtype=torch.float32)
        out = torch.empty(2, device=x.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dl = torch.empty_like(logits) if need else None
        with _timed('image_recon', 0.0, 4.0 * count * (3 if need else 2)):
            _lib.check(lib.arvae_image_recon(_ptr(logits), _ptr(x), count, batch, dist, _ptr(ws), _ptr(out),
                                             _ptr(dl), _stream()), 'image_recon')
        if need:
            ctx.save_for_backward(dl)
        loss, acc = out[0], out[1]
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_acc):
        (dl,) = ctx.saved_tensors
        return scale_by_scalar(g, dl), None, None


def image_recon(logits, x, dist='bernoulli'):
    """-> (sum_all(term)/batch, pixel accuracy)."""
    if dist not in RECON_DIST:
        raise AttributeError('invalid dist')
    return _ImageReconFn.apply(logits.contiguous(), x.contiguous(), RECON_DIST[dist])


class _TokenReconFn(Function):
    @staticmethod
    def forward(ctx, weights, targets):
        _dev(weights, targets)
        lib = _lib.load()
        vocab = weights.shape[-1]
        rows = weights.numel() // vocab
        ws = torch.empty(lib.arvae_recon_ws_floats(rows), device=weights.device, dtype=torch.float32)
        out = torch.empty(2, device=weights.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dw = torch.empty_like(weights) if need else None
        _lib.check(lib.arvae_token_recon(_ptr(weights), _ptr(targets), rows, vocab, _ptr(ws), _ptr(out), _ptr(dw),
                                         _stream()), 'token_recon')
        if need:
            ctx.save_for_backward(dw)
        loss, acc = out[0], out[1]
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_acc):
        (dw,) = ctx.saved_tensors
        return scale_by_scalar(g, dw), None


def token_recon(weights, targets):
    """-> (mean cross entropy over rows, top-1 accuracy) for weights [..., V], int64 targets [...]."""
    if targets.dtype != torch.int64:
        raise TypeError('targets must be int64')
    return _TokenReconFn.apply(weights.contiguous(), targets.contiguous())


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, zero_grad=False, status=None):
    """one Adam update of the flat arenas; zero_grad: g is cleared by the same kernel once it has been consumed;
    status (int32 device tensor of >= 5 words, optional): while status[0] != 0 the launch leaves p, m, v alone and counts
    the skipped update in status[4] (include/arvae_hip.h, arvae_adam_step)"""
    _dev(p, g, m, v)
    lib = _lib.load()
    with _timed('adam', 0.0, 28.0 * p.numel()):
        _lib.check(lib.arvae_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(step), lr, beta1, beta2,
                                       eps, grad_scale, int(bool(zero_grad)), _ptr(status), _stream()), 'adam_step')


# ------------------------------------------------------------------------------------------------
# MeasureVAE building blocks (GRU gate math, embedding, concat/split, masks, argmax, attribute labels)
# ------------------------------------------------------------------------------------------------
class _GruGatesFn(Function):
    """h' = GRU cell gates given gi = W_ih x + b_ih and gh = W_hh h + b_hh ([B, 3H], gate order r|z|n)."""

    @staticmethod
    def forward(ctx, gi, gh, h_prev):
        _dev(gi, gh, h_prev)
        lib = _lib.load()
        b, h3 = gi.shape
        hid = h3 // 3
        h_new = torch.empty(b, hid, device=gi.device, dtype=torch.float32)
        saved = torch.empty(4, b, hid, device=gi.device, dtype=torch.float32)
        _lib.check(lib.arvae_gru_gates_fwd(_ptr(gi), _ptr(gh), _ptr(h_prev), b, hid, _ptr(h_new), _ptr(saved),
                                           _stream()), 'gru_gates_fwd')
        ctx.save_for_backward(saved, h_prev)
        ctx.dims = (b, hid)
        return h_new

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        saved, h_prev = ctx.saved_tensors
        lib = _lib.load()
        b, hid = ctx.dims
        dh = dh.contiguous()
        dgi = torch.empty(b, 3 * hid, device=dh.device, dtype=torch.float32)
        dgh = torch.empty_like(dgi)
        dhp = torch.empty(b, hid, device=dh.device, dtype=torch.float32)
        _lib.check(lib.arvae_gru_gates_bwd(_ptr(dh), _ptr(saved), _ptr(h_prev), b, hid, _ptr(dgi), _ptr(dgh), _ptr(dhp),
                                           _stream()), 'gru_gates_bwd')
        return dgi, dgh, (dhp if h_prev is not None else None)


def gru_gates(gi, gh, h_prev=None):
    return _GruGatesFn.apply(gi.contiguous(), gh.contiguous(), None if h_prev is None else h_prev.contiguous())


def gru_sequence_supported(hidden):
    return bool(_lib.load().arvae_gru_seq_supported(int(hidden)))


def gru_sequence_wide_supported(hidden):
    """the streamed-weights recurrences (csrc/gru_wide.hip: one launch per time step): hidden sizes 256 and 512"""
    return bool(_lib.load().arvae_gru_seq_wide_supported(int(hidden)))


def _gru_seq_descs(n):
    return (_lib.GruSeqDesc * n)()


def _gru_seq_call(lib, which, descs, ndir, steps, rows, hid, dev):
    """_GruSeqFn's library call: arvae_gru_seq_<which> (resident weights, one launch) or, at a wide hidden size,
    arvae_gru_seq_wide_<which> (one launch per time step inside the call) with its scratch"""
    if not lib.arvae_gru_seq_wide_supported(hid):
        return getattr(lib, 'arvae_gru_seq_' + which)(descs, ndir, steps, rows, hid, _stream())
    n_ws = lib.arvae_gru_seq_wide_ws_floats(ndir, rows, hid)
    if n_ws < 0:
        raise RuntimeError(f'gru_seq_wide_{which}: {ndir} sequences of {rows} rows at hidden size {hid}')
    ws = torch.empty(max(int(n_ws), 4), device=dev, dtype=torch.float32)
    return getattr(lib, 'arvae_gru_seq_wide_' + which)(descs, ndir, steps, rows, hid, _ptr(ws), _stream())


class _GruSeqFn(Function):
    """All time steps of one GRU layer (1..4 directions / parameter sets) in one launch; see csrc/gru_seq.hip.

    per direction d the inputs are gi_d (T, R, 3H) -- or (R, 3H) when the same projection feeds every step --,
    w_hh_d, b_hh_d, h0_d (R, H) or None.  With gi_merged (T, R, ndir*3H) the directions read their input projection from
    columns [3H d, 3H (d+1)) of that ONE tensor (both directions of a bidirectional layer projected by one GEMM,
    dense_pair) and the per-direction gi_d are None; its gradient comes back as one tensor as well.
    Outputs: (T, R, ndir*H) with direction d in columns [dH, (d+1)H), and the final states (R, ndir*H) = nn.GRU's h_n (each
    direction's last processed step), written by the sequence launch itself."""

    @staticmethod
    def forward(ctx, steps, reverse, want_finals, gi_merged, *tensors):
        ndir = len(reverse)
        gis, whs, bhs, h0s = tensors[0::4], tensors[1::4], tensors[2::4], tensors[3::4]
        _dev(*[t for t in tensors if t is not None])
        lib = _lib.load()
        hid = whs[0].shape[1]
        rows = gi_merged.shape[1] if gi_merged is not None else gis[0].shape[-2]
        dev = whs[0].device
        out = torch.empty(steps, rows, ndir * hid, device=dev, dtype=torch.float32)
        saved = torch.empty(ndir, steps, rows, 4 * hid, device=dev, dtype=torch.float32)
        finals = torch.empty(rows, ndir * hid, device=dev, dtype=torch.float32) if want_finals else None
        descs = _gru_seq_descs(ndir)
        for d in range(ndir):
            q = descs[d]
            if gi_merged is not None:
                q.gi = gi_merged.data_ptr() + 4 * d * 3 * hid
                q.gi_tstride, q.gi_rstride = rows * ndir * 3 * hid, ndir * 3 * hid
            else:
                q.gi, q.gi_tstride = _ptr(gis[d]), (rows * 3 * hid if gis[d].dim() == 3 else 0)
            q.w_hh, q.b_hh, q.h0 = _ptr(whs[d]), _ptr(bhs[d]), _ptr(h0s[d])
            q.h_all, q.h_stride = out.data_ptr() + 4 * d * hid, ndir * hid
            q.saved, q.reverse = saved[d].data_ptr(), int(reverse[d])
            if finals is not None:
                q.h_fin, q.h_fin_stride = finals.data_ptr() + 4 * d * hid, ndir * hid
        with _timed('gru_seq_fwd', 2.0 * ndir * steps * rows * 3 * hid * hid, 4.0 * ndir * steps * rows * 8 * hid):
            _lib.check(_gru_seq_call(lib, 'fwd', descs, ndir, steps, rows, hid, dev), 'gru_seq_fwd')
        ctx.save_for_backward(out, saved, *whs, *[h for h in h0s if h is not None])
        ctx.h0_present = [h is not None for h in h0s]
        ctx.gi_const = [g is not None and g.dim() == 2 for g in gis]
        ctx.merged = gi_merged is not None
        ctx.refs = (whs, bhs)
        ctx.geom = (steps, rows, hid, tuple(reverse))
        ctx.set_materialize_grads(False)
        if not want_finals:
            none = out.new_empty(0)                              # (an empty tensor: no launch)
            ctx.mark_non_differentiable(none)
            return out, none
        return out, finals

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_fin):
        steps, rows, hid, reverse = ctx.geom
        ndir = len(reverse)
        out, saved = ctx.saved_tensors[:2]
        whs = ctx.saved_tensors[2:2 + ndir]
        h0_it = iter(ctx.saved_tensors[2 + ndir:])
        h0s = [next(h0_it) if p else None for p in ctx.h0_present]
        lib = _lib.load()
        dev = out.device
        d_out = None if d_out is None else d_out.contiguous()
        d_fin = None if (d_fin is None or d_fin.numel() == 0) else d_fin.contiguous()
        if ctx.merged:                                           # one (T, R, ndir * 3H) gradient for the one projection
            dgi_all = torch.empty(steps, rows, ndir * 3 * hid, device=dev, dtype=torch.float32)
            dgi = None
        else:
            dgi_all = None
            dgi = torch.empty(ndir, steps, rows, 3 * hid, device=dev, dtype=torch.float32)
        dgh = torch.empty(ndir, steps, rows, 3 * hid, device=dev, dtype=torch.float32)
        h_prev = torch.empty(ndir, steps, rows, hid, device=dev, dtype=torch.float32)
        base = 4                                                 # inputs: steps, reverse, want_finals, gi_merged, then 4 per direction
        dh0 = [torch.empty(rows, hid, device=dev, dtype=torch.float32)
               if (h0s[d] is not None and ctx.needs_input_grad[base + 4 * d + 3]) else None for d in range(ndir)]
        descs = _gru_seq_descs(ndir)
        for d in range(ndir):
            q = descs[d]
            q.w_hh, q.h0 = _ptr(whs[d]), _ptr(h0s[d])
            q.h_all, q.h_stride = out.data_ptr() + 4 * d * hid, ndir * hid
            q.saved, q.reverse = saved[d].data_ptr(), int(reverse[d])
            if d_out is not None:
                q.dh_all, q.dh_stride = d_out.data_ptr() + 4 * d * hid, ndir * hid
            if d_fin is not None:
                q.dh_last, q.dh_last_stride = d_fin.data_ptr() + 4 * d * hid, ndir * hid
            if ctx.merged:
                q.dgi, q.dgi_rstride = dgi_all.data_ptr() + 4 * d * 3 * hid, ndir * 3 * hid
            else:
                q.dgi = dgi[d].data_ptr()
            q.dgh, q.dh0 = dgh[d].data_ptr(), _ptr(dh0[d])
            q.h_prev_out = h_prev[d].data_ptr()
        with _timed('gru_seq_bwd', 2.0 * ndir * steps * rows * 3 * hid * hid, 4.0 * ndir * steps * rows * 12 * hid):
            _lib.check(_gru_seq_call(lib, 'bwd', descs, ndir, steps, rows, hid, dev), 'gru_seq_bwd')
        grads = [None, None, None, dgi_all if (ctx.merged and ctx.needs_input_grad[3]) else None]
        link = Link.dense(hid, 3 * hid)
        w_refs, b_refs = ctx.refs
        for d in range(ndir):
            d_w = d_b = None
            if ctx.needs_input_grad[base + 4 * d + 1]:
                buf, direct = _grad_target(w_refs[d])
                bbuf, bdirect = _grad_target(b_refs[d])
                link_wgrad(link, steps * rows, _operand(dgh[d].view(steps * rows, 3 * hid)),
                           _operand(h_prev[d].view(steps * rows, hid)), buf, bbuf, 1)
                d_w, d_b = (None if direct else buf), (None if bdirect else bbuf)
            g_gi = None
            if not ctx.merged and ctx.needs_input_grad[base + 4 * d]:
                g_gi = dgi[d].sum(0) if ctx.gi_const[d] else dgi[d]
            grads += [g_gi, d_w, d_b, dh0[d]]
        return tuple(grads)


def gru_sequence(steps, directions, finals=True, merged_gi=None):
    """directions: list of (gi, w_hh, b_hh, h0, reverse) -> (outputs (T, R, ndir*H), final states (R, ndir*H) or, with
    finals=False, None).  merged_gi (T, R, ndir*3H): the directions' input projections as one tensor (their gi entries None)."""
    flat = []
    for gi, w_hh, b_hh, h0, _ in directions:
        flat += [None if gi is None else gi.contiguous(), w_hh, b_hh, None if h0 is None else h0.contiguous()]
    out, fin = _GruSeqFn.apply(int(steps), tuple(bool(d[4]) for d in directions), bool(finals),
                               None if merged_gi is None else merged_gi.contiguous(), *flat)
    return out, (fin if finals else None)


def _adjacent(a, b):
    """b starts where a ends, in the same allocation (two parameters of the trainer's flat arena laid out back to back)"""
    return (a is not None and b is not None and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and a.data_ptr() + a.numel() * a.element_size() == b.data_ptr())


class _DensePairFn(Function):
    """two Linear layers (+ one activation) on the same input whose weights (and biases) are adjacent in memory, as one
    [out_a + out_b, in] layer"""

    @staticmethod
    def forward(ctx, x, w_a, w_b, b_a, b_b, act):
        _dev(x, w_a, w_b, b_a, b_b)
        n, n_in, n_out = x.shape[0], w_a.shape[1], w_a.shape[0] + w_b.shape[0]
        link = Link.dense(n_in, n_out)
        w_cat = w_a.detach().as_strided((n_out, n_in), (n_in, 1))
        b_cat = b_a.detach().as_strided((n_out,), (1,))
        out = link_down(link, n, _operand(x), w_cat, b_cat, act, None)
        ctx.link, ctx.n, ctx.act = link, n, act
        ctx.save_for_backward(x, w_cat, out)
        ctx.refs = (w_a, w_b, b_a, b_b)
        ctx.x_ref = x if (x.is_leaf and x.requires_grad) else None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w_cat, out = ctx.saved_tensors
        link, n = ctx.link, ctx.n
        g = g.contiguous()
        gop, keep = _plain_gradient(g, out, None, ctx.act, link, n)
        d_x = link_up(link, n, gop, w_cat, None, ACT_NONE, None) if ctx.needs_input_grad[0] else None
        x_ref = ctx.x_ref
        if d_x is not None and x_ref is not None and x_ref.grad is not None and x_ref.grad.shape == d_x.shape:
            # the input is itself a parameter with a gradient buffer (an embedding table projected as a whole): added here, on
            # this stream, instead of by an AccumulateGrad node (whose stream is not the capture's: graphed.py)
            _grad_target(x_ref)
            x_ref.grad.add_(d_x)
            d_x = None
        w_a, w_b, b_a, b_b = ctx.refs
        if ctx.needs_input_grad[1]:
            _grad_target(w_a), _grad_target(b_a)                 # (the arena is written without autograd's accumulation)
            n_out, n_in = w_cat.shape
            gw = w_a.grad.as_strided((n_out, n_in), (n_in, 1))
            gb = b_a.grad.as_strided((n_out,), (1,))
            if not _defer_dense_wgrad(link, n, gop, (g, keep, out, x), x, gw, gb):
                link_wgrad(link, n, gop, _operand(x), gw, gb, 1)
        return d_x, None, None, None, None, None


def dense_pair(x, w_a, b_a, w_b, b_b, act=ACT_NONE):
    """act(x (n, in) times [w_a; w_b]^T + [b_a; b_b]) as ONE product -> (n, out_a + out_b) when the two layers' weights, biases
    and (when gradients are on) gradient buffers sit back to back in memory -- the trainer's flat arena in
    Model.arena_parameters() order -- ; None when they do not (the caller runs the layers one by one)."""
    if not (_adjacent(w_a, w_b) and _adjacent(b_a, b_b) and w_a.shape[1] == w_b.shape[1]):
        return None
    if torch.is_grad_enabled() and (w_a.requires_grad or w_b.requires_grad):
        if not (w_a.requires_grad and w_b.requires_grad and _adjacent(w_a.grad, w_b.grad) and _adjacent(b_a.grad, b_b.grad)):
            return None
    return _DensePairFn.apply(x, w_a, w_b, b_a, b_b, int(act))


def tick_free_run_supported(hidden, vocab):
    """True when the one-launch free-running tick decoder is built for (hidden, vocab); else go tick by tick."""
    return bool(_lib.load().arvae_tick_free_run_supported(int(hidden), int(vocab)))


def sample_filter(vocab, top_k=None, top_p=None, allow=None):
    """-> (_lib.SampleFilter, the tensors it points into) for arvae_*_filtered over rows of `vocab` notes: top_k None or 0 = off, top_p
    None or 1 = off, allow None or a uint8 device tensor (vocab,) of the notes that may be emitted.  The ranges are the library's to
    check (ARVAE_E_INVALID -> RuntimeError); HierarchicalDecoder.generate validates on the host first."""
    if allow is not None:
        if allow.dtype != torch.uint8 or tuple(allow.shape) != (vocab,):
            raise ValueError(f'the allowed-note mask must be uint8 of shape ({vocab},), got {allow.dtype} {tuple(allow.shape)}')
        _dev(allow)
        allow = allow.contiguous()
    return _lib.SampleFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p), _ptr(allow)), allow


def tick_free_run_filtered(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, uniforms, temperature=1.0, top_k=None,
                           top_p=None, allow=None):
    """tick_free_run's sampled pass over the notes a top-k cut, a nucleus cut and a note mask leave (arvae_tick_free_run_filtered;
    the semantics: include/arvae_hip.h, arvae_sample_filter_t).  No keep-masks: generation runs with dropout off."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab, uniforms)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    flt, allow = sample_filter(vocab, top_k, top_p, allow)
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    tokens = torch.empty(batch, beats * ticks_per_beat, device=gib.device, dtype=torch.int64)
    ws = torch.empty(lib.arvae_tick_free_run_ws_floats(hid), device=gib.device, dtype=torch.float32)
    u = _sampling_uniforms(uniforms, (batch, beats * ticks_per_beat))
    with _timed('tick_free_run_filtered', 2.0 * batch * beats * ticks_per_beat * (9 * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_free_run_filtered(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), None, 1.0, batch,
                                                    beats, ticks_per_beat, hid, vocab, _ptr(u), 1.0 / float(temperature),
                                                    ctypes.byref(flt), _ptr(tokens), _ptr(ws), _stream()), 'tick_free_run_filtered')
    return tokens


def tick_free_run(weights, h0_l0, h0_l1, gib, ptab, mask, keep_scale, batch, beats, ticks_per_beat, uniforms=None, temperature=1.0):
    """tokens (B, beats*ticks_per_beat) int64 of the free-running tick decoder; no autograd (csrc/tick_decoder.hip).
    weights = (w_hh0, b_hh0, w_ih1, b_ih1, w_hh1, b_hh1, w_out, b_out).
    uniforms None: the top-1 note is fed back (arvae_tick_free_run).  uniforms (B, beats*ticks_per_beat) float32 in (0, 1]: the note
    drawn from softmax(logits / temperature) by inverting its CDF at that tick's uniform (arvae_tick_free_run_sampled)."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab, mask, uniforms)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    tokens = torch.empty(batch, beats * ticks_per_beat, device=gib.device, dtype=torch.int64)
    ws = torch.empty(lib.arvae_tick_free_run_ws_floats(hid), device=gib.device, dtype=torch.float32)
    with _timed('tick_free_run', 2.0 * batch * beats * ticks_per_beat * (9 * hid * hid + vocab * hid), 0.0):
        if uniforms is None:
            _lib.check(lib.arvae_tick_free_run(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), _ptr(mask),
                                               float(keep_scale), batch, beats, ticks_per_beat, hid, vocab, _ptr(tokens),
                                               _ptr(ws), _stream()), 'tick_free_run')
        else:
            u = _sampling_uniforms(uniforms, (batch, beats * ticks_per_beat))
            _lib.check(lib.arvae_tick_free_run_sampled(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), _ptr(mask),
                                                       float(keep_scale), batch, beats, ticks_per_beat, hid, vocab, _ptr(u),
                                                       1.0 / float(temperature), _ptr(tokens), _ptr(ws), _stream()),
                       'tick_free_run_sampled')
    return tokens


def tick_free_run_wide_supported(hidden, vocab):
    """True when the streamed-weights free-running tick decoder (csrc/tick_wide.hip: three launches per tick inside one call) is built
    for (hidden, vocab): hidden 256 or 512, 2 to 128 notes"""
    return bool(_lib.load().arvae_tick_free_run_wide_supported(int(hidden), int(vocab)))


def tick_free_run_wide(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, mask=None, keep_scale=1.0, uniforms=None,
                       temperature=1.0, filter=None, plan=None, return_logits=False):
    """tokens (B, beats*ticks_per_beat) int64 of the free-running two-layer tick decoder at hidden 256 / 512 (arvae_tick_free_run_wide;
    the picks: include/arvae_hip.h).  weights / h0 / gib / ptab / mask as tick_free_run.  uniforms None: argmax; uniforms alone: the
    multinomial draw; filter = (top_k, top_p, allow) as tick_free_run_filtered; plan (with filter = (top_k, top_p)) as
    tick_free_run_planned.  return_logits: -> (tokens, logits (B, ticks, V)), the logits every pick was made from."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab, mask, uniforms)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    ticks, dev = beats * ticks_per_beat, gib.device
    flt = npl = None
    if filter is not None or plan is not None:
        top_k, top_p, allow = (tuple(filter) + (None,) * 3)[:3] if filter is not None else (None, None, None)
        flt, allow = sample_filter(vocab, top_k, top_p, allow)
    if plan is not None:
        npl, plan = note_plan(plan, batch, ticks, vocab)
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (ticks, batch, hid)):
        raise ValueError(f'the keep-mask must be uint8 of shape {(ticks, batch, hid)}, got {mask.dtype} {tuple(mask.shape)}')
    u = None if uniforms is None else _sampling_uniforms(uniforms, (batch, ticks))
    n_ws = lib.arvae_tick_free_run_wide_ws_floats(batch, hid, vocab)
    if n_ws < 0:
        raise RuntimeError(f'tick_free_run_wide: {batch} rows at hidden size {hid} and {vocab} notes')
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    tokens = torch.empty(batch, ticks, device=dev, dtype=torch.int64)
    logits = torch.empty(batch, ticks, vocab, device=dev, dtype=torch.float32) if return_logits else None
    ws = torch.empty(int(n_ws), device=dev, dtype=torch.float32)
    with _timed('tick_free_run_wide', 2.0 * batch * ticks * (9 * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_free_run_wide(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), _ptr(mask),
                                                float(keep_scale), batch, beats, ticks_per_beat, hid, vocab, _ptr(u),
                                                1.0 / float(temperature), None if flt is None else ctypes.byref(flt),
                                                None if npl is None else ctypes.byref(npl), _ptr(tokens), _ptr(logits), _ptr(ws),
                                                _stream()), 'tick_free_run_wide')
    return (tokens, logits) if return_logits else tokens


def tick_free_run_layers_supported(hidden, vocab, layers):
    """True when the one-launch free-running tick decoder is built for a `layers`-deep tick RNN other than the two-layer one
    (tick_free_run_supported / tick_free_run); else go tick by tick."""
    return bool(_lib.load().arvae_tick_free_run_layers_supported(int(hidden), int(vocab), int(layers)))


def _tick_stack(cells, w_out, b_out, h0, gib, ptab, batch, ticks):
    """-> (_lib.TickStack of a GRU stack, the contiguous initial states it points into, tokens, workspace) for the layers calls"""
    layers = len(cells)
    if len(h0) != layers or layers > _lib.TICK_MAX_LAYERS:
        raise ValueError(f'{layers} layers need {layers} initial states (at most {_lib.TICK_MAX_LAYERS} layers)')
    h0 = [s.contiguous() for s in h0]
    _dev(*[t for c in cells for t in c], w_out, b_out, *h0, gib, ptab)
    hid = cells[0][1].shape[1]
    ts = _lib.TickStack()
    ts.layers = layers
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(cells):
        ts.w_ih[l], ts.w_hh[l], ts.b_ih[l], ts.b_hh[l], ts.h0[l] = _ptr(w_ih), _ptr(w_hh), _ptr(b_ih), _ptr(b_hh), _ptr(h0[l])
    ts.w_out, ts.b_out, ts.h0_stride = _ptr(w_out), _ptr(b_out), 0
    tokens = torch.empty(batch, ticks, device=gib.device, dtype=torch.int64)
    ws = torch.empty(_lib.load().arvae_tick_free_run_layers_ws_floats(hid, layers), device=gib.device, dtype=torch.float32)
    return ts, h0, tokens, ws


def tick_free_run_layers(cells, w_out, b_out, h0, gib, ptab, mask, keep_scale, batch, beats, ticks_per_beat, uniforms=None,
                         temperature=1.0):
    """tick_free_run for a GRU stack of len(cells) layers (arvae_tick_free_run_layers): cells[l] = (w_ih, w_hh, b_ih, b_hh) of layer l
    (layer 0's input weights are not read: gib / ptab hold their products), h0 = the layers' initial states (beats*B, H) each,
    mask None or uint8 (layers-1, beats*ticks_per_beat, B, H), one keep-mask per layer boundary."""
    layers, ticks = len(cells), beats * ticks_per_beat
    ts, h0, tokens, ws = _tick_stack(cells, w_out, b_out, h0, gib, ptab, batch, ticks)
    _dev(mask, uniforms)
    lib = _lib.load()
    hid, vocab = cells[0][1].shape[1], w_out.shape[0]
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (layers - 1, ticks, batch, hid)):
        raise ValueError(f'keep-masks must be uint8 of shape {(layers - 1, ticks, batch, hid)}, got {mask.dtype} {tuple(mask.shape)}')
    u = None if uniforms is None else _sampling_uniforms(uniforms, (batch, ticks))
    mask = None if mask is None else mask.contiguous()
    with _timed('tick_free_run_layers', 2.0 * batch * ticks * (3 * (2 * layers - 1) * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_free_run_layers(ctypes.byref(ts), _ptr(gib), _ptr(ptab), _ptr(mask), float(keep_scale), batch, beats,
                                                  ticks_per_beat, hid, vocab, _ptr(u), 1.0 / float(temperature), _ptr(tokens),
                                                  _ptr(ws), _stream()), 'tick_free_run_layers')
    return tokens


def tick_free_run_layers_filtered(cells, w_out, b_out, h0, gib, ptab, batch, beats, ticks_per_beat, uniforms, temperature=1.0, top_k=None,
                                  top_p=None, allow=None):
    """tick_free_run_filtered for a GRU stack of 1, 3 or 4 layers (arvae_tick_free_run_layers_filtered).  No keep-masks."""
    layers, ticks = len(cells), beats * ticks_per_beat
    ts, h0, tokens, ws = _tick_stack(cells, w_out, b_out, h0, gib, ptab, batch, ticks)
    _dev(uniforms)
    lib = _lib.load()
    hid, vocab = cells[0][1].shape[1], w_out.shape[0]
    flt, allow = sample_filter(vocab, top_k, top_p, allow)
    u = _sampling_uniforms(uniforms, (batch, ticks))
    with _timed('tick_free_run_layers_filtered', 2.0 * batch * ticks * (3 * (2 * layers - 1) * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_free_run_layers_filtered(ctypes.byref(ts), _ptr(gib), _ptr(ptab), None, 1.0, batch, beats, ticks_per_beat,
                                                           hid, vocab, _ptr(u), 1.0 / float(temperature), ctypes.byref(flt),
                                                           _ptr(tokens), _ptr(ws), _stream()), 'tick_free_run_layers_filtered')
    return tokens


def _beam_mask(vocab, allow):
    """-> (the mask on the device or None, the number of notes it allows): the library takes the count from the host"""
    if allow is None:
        return None, int(vocab)
    if allow.dtype != torch.uint8 or tuple(allow.shape) != (vocab,):
        raise ValueError(f'the allowed-note mask must be uint8 of shape ({vocab},), got {allow.dtype} {tuple(allow.shape)}')
    _dev(allow)
    return allow.contiguous(), int(allow.count_nonzero())


def tick_beam_search_supported(hidden, vocab, width):
    """True when the one-launch beam search is offered for (hidden, vocab, width); else go tick by tick (beam_select)."""
    return bool(_lib.load().arvae_tick_beam_search_supported(int(hidden), int(vocab), int(width)))


def tick_beam_search(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, width, allow=None, allowed=None):
    """the beam search of the two-layer tick decoder in one launch (arvae_tick_beam_search; the semantics: include/arvae_hip.h, "Beam
    search"): -> (parents (B, T, W) int32, tokens (B, T, W) int64, scores_hist (B, T, W), sequences (B, W, T) int64, scores (B, W)).
    weights / h0 / gib / ptab as tick_free_run; allow None or uint8 (V,) on the device (allowed: its count, when the caller has it)."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    allow, count = _beam_mask(vocab, allow) if allowed is None or allow is None else (allow.contiguous(), int(allowed))
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    ticks, dev = beats * ticks_per_beat, gib.device
    parents = torch.empty(batch, ticks, width, device=dev, dtype=torch.int32)
    tokens = torch.empty(batch, ticks, width, device=dev, dtype=torch.int64)
    hist = torch.empty(batch, ticks, width, device=dev, dtype=torch.float32)
    seqs = torch.empty(batch, width, ticks, device=dev, dtype=torch.int64)
    scores = torch.empty(batch, width, device=dev, dtype=torch.float32)
    ws = torch.empty(lib.arvae_tick_beam_search_ws_floats(hid), device=dev, dtype=torch.float32)
    with _timed('tick_beam_search', 2.0 * batch * width * ticks * (9 * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_beam_search(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), batch, beats,
                                              ticks_per_beat, hid, vocab, int(width), _ptr(allow), count, _ptr(parents), _ptr(tokens),
                                              _ptr(hist), _ptr(seqs), _ptr(scores), _ptr(ws), _stream()), 'tick_beam_search')
    return parents, tokens, hist, seqs, scores


def beam_select(logits, scores, live, allow=None, allowed=None):
    """one tick's selection of the beam search on given logits (codes * W, V) and scores (codes, W), the first `live` beams of a code
    live (arvae_beam_select) -> (parents (codes, W) int32, notes (codes, W) int64, scores (codes, W))."""
    _dev(logits, scores)
    lib = _lib.load()
    logits, scores = logits.contiguous(), scores.contiguous()
    codes, width = scores.shape
    vocab = logits.shape[1]
    if logits.shape[0] != codes * width or scores.dtype != torch.float32 or logits.dtype != torch.float32:
        raise ValueError(f'beam_select takes float32 logits ({codes * width}, V) for scores ({codes}, {width}), got {tuple(logits.shape)}')
    allow, count = _beam_mask(vocab, allow) if allowed is None or allow is None else (allow.contiguous(), int(allowed))
    parents = torch.empty(codes, width, device=logits.device, dtype=torch.int32)
    notes = torch.empty(codes, width, device=logits.device, dtype=torch.int64)
    out = torch.empty(codes, width, device=logits.device, dtype=torch.float32)
    _lib.check(lib.arvae_beam_select(_ptr(logits), _ptr(scores), codes, width, vocab, int(live), _ptr(allow), count, _ptr(parents),
                                     _ptr(notes), _ptr(out), _stream()), 'beam_select')
    return parents, notes, out


def sequence_log_prob(weights, tokens, allow=None):
    """(R,) float32: the sum over t of the log-softmax of weights (R, T, V) over the allowed notes at tokens (R, T) int64
    (arvae_sequence_log_prob); a token that is not allowed gives -inf."""
    _dev(weights, tokens)
    lib = _lib.load()
    if weights.dim() != 3 or tuple(tokens.shape) != tuple(weights.shape[:2]) or tokens.dtype != torch.int64 or weights.dtype != torch.float32:
        raise ValueError(f'sequence_log_prob takes float32 weights (R, T, V) and int64 tokens (R, T), got {tuple(weights.shape)} '
                         f'{weights.dtype} and {tuple(tokens.shape)} {tokens.dtype}')
    weights, tokens = weights.contiguous(), tokens.contiguous()
    rows, steps, vocab = weights.shape
    allow, _ = _beam_mask(vocab, allow)
    out = torch.empty(rows, device=weights.device, dtype=torch.float32)
    _lib.check(lib.arvae_sequence_log_prob(_ptr(weights), _ptr(tokens), rows, steps, vocab, _ptr(allow), _ptr(out), _stream()),
               'sequence_log_prob')
    return out


# ---- note plans: an allowed-note mask per (row, tick) (include/arvae_hip.h, arvae_note_plan_t) -----------------------------------
def note_plan(plan, rows, ticks, vocab):
    """-> (_lib.NotePlan, the tensor it points into) of a plan on the device: uint8 (rows, ticks, vocab), or (ticks, vocab) = the same
    plan for every row (row stride 0).  Emptiness and the flags' values are the host validator's to check
    (HierarchicalDecoder.note_plan): the kernels return a note in range for any bytes."""
    if plan.dtype != torch.uint8 or tuple(plan.shape) not in ((rows, ticks, vocab), (ticks, vocab)):
        raise ValueError(f'a note plan must be uint8 of shape ({rows}, {ticks}, {vocab}) or ({ticks}, {vocab}), got {plan.dtype} '
                         f'{tuple(plan.shape)}')
    _dev(plan)
    plan = plan.contiguous()
    return _lib.NotePlan(_ptr(plan), ticks * vocab if plan.dim() == 3 else 0, vocab), plan


def tick_free_run_planned(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, uniforms, plan, temperature=1.0, top_k=None,
                          top_p=None):
    """tick_free_run_filtered with the allowed notes given per (row, tick) by `plan` (arvae_tick_free_run_planned; `note_plan`).
    top_k = 1 is the plan's argmax: the draws are then without effect."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab, uniforms)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    ticks = beats * ticks_per_beat
    flt, _ = sample_filter(vocab, top_k, top_p, None)
    npl, plan = note_plan(plan, batch, ticks, vocab)
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    tokens = torch.empty(batch, ticks, device=gib.device, dtype=torch.int64)
    ws = torch.empty(lib.arvae_tick_free_run_ws_floats(hid), device=gib.device, dtype=torch.float32)
    u = _sampling_uniforms(uniforms, (batch, ticks))
    with _timed('tick_free_run_planned', 2.0 * batch * ticks * (9 * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_free_run_planned(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), None, 1.0, batch,
                                                   beats, ticks_per_beat, hid, vocab, _ptr(u), 1.0 / float(temperature),
                                                   ctypes.byref(flt), ctypes.byref(npl), _ptr(tokens), _ptr(ws), _stream()),
                   'tick_free_run_planned')
    return tokens


def tick_free_run_layers_planned(cells, w_out, b_out, h0, gib, ptab, batch, beats, ticks_per_beat, uniforms, plan, temperature=1.0,
                                 top_k=None, top_p=None):
    """tick_free_run_planned for a GRU stack of 1, 3 or 4 layers (arvae_tick_free_run_layers_planned)."""
    layers, ticks = len(cells), beats * ticks_per_beat
    ts, h0, tokens, ws = _tick_stack(cells, w_out, b_out, h0, gib, ptab, batch, ticks)
    _dev(uniforms)
    lib = _lib.load()
    hid, vocab = cells[0][1].shape[1], w_out.shape[0]
    flt, _ = sample_filter(vocab, top_k, top_p, None)
    npl, plan = note_plan(plan, batch, ticks, vocab)
    u = _sampling_uniforms(uniforms, (batch, ticks))
    with _timed('tick_free_run_layers_planned', 2.0 * batch * ticks * (3 * (2 * layers - 1) * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_free_run_layers_planned(ctypes.byref(ts), _ptr(gib), _ptr(ptab), None, 1.0, batch, beats, ticks_per_beat,
                                                          hid, vocab, _ptr(u), 1.0 / float(temperature), ctypes.byref(flt),
                                                          ctypes.byref(npl), _ptr(tokens), _ptr(ws), _stream()),
                   'tick_free_run_layers_planned')
    return tokens


def row_sample_planned(w, u, plan, tick, temperature=1.0, top_k=None, top_p=None):
    """row_sample_filtered with row r's allowed notes those of plan[r, tick] (arvae_row_sample_planned): the tick-by-tick path."""
    _dev(w, u)
    lib = _lib.load()
    w = w.contiguous()
    rows, cols = w.shape
    u = _sampling_uniforms(u, (rows,))
    ticks = plan.shape[-2]
    flt, _ = sample_filter(cols, top_k, top_p, None)
    npl, plan = note_plan(plan, rows, ticks, cols)
    idx = torch.empty(rows, device=w.device, dtype=torch.int64)
    _lib.check(lib.arvae_row_sample_planned(_ptr(w), rows, cols, _ptr(u), 1.0 / float(temperature), ctypes.byref(flt), ctypes.byref(npl),
                                            ticks, int(tick), _ptr(idx), _stream()), 'row_sample_planned')
    return idx


def tick_beam_search_planned(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, width, plan):
    """tick_beam_search under a note plan (arvae_tick_beam_search_planned): the same five tensors; slots without a finite candidate are
    dead (score -inf, listed last, their tokens inside the plan)."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    ticks, dev = beats * ticks_per_beat, gib.device
    npl, plan = note_plan(plan, batch, ticks, vocab)
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    parents = torch.empty(batch, ticks, width, device=dev, dtype=torch.int32)
    tokens = torch.empty(batch, ticks, width, device=dev, dtype=torch.int64)
    hist = torch.empty(batch, ticks, width, device=dev, dtype=torch.float32)
    seqs = torch.empty(batch, width, ticks, device=dev, dtype=torch.int64)
    scores = torch.empty(batch, width, device=dev, dtype=torch.float32)
    ws = torch.empty(lib.arvae_tick_beam_search_ws_floats(hid), device=dev, dtype=torch.float32)
    with _timed('tick_beam_search_planned', 2.0 * batch * width * ticks * (9 * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_beam_search_planned(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), batch, beats,
                                                      ticks_per_beat, hid, vocab, int(width), ctypes.byref(npl), _ptr(parents),
                                                      _ptr(tokens), _ptr(hist), _ptr(seqs), _ptr(scores), _ptr(ws), _stream()),
                   'tick_beam_search_planned')
    return parents, tokens, hist, seqs, scores


def beam_select_planned(logits, scores, live, plan, tick):
    """beam_select with code b's allowed notes those of plan[b, tick] (arvae_beam_select_planned); no count: slots without a candidate
    are dead."""
    _dev(logits, scores)
    lib = _lib.load()
    logits, scores = logits.contiguous(), scores.contiguous()
    codes, width = scores.shape
    vocab = logits.shape[1]
    if logits.shape[0] != codes * width or scores.dtype != torch.float32 or logits.dtype != torch.float32:
        raise ValueError(f'beam_select takes float32 logits ({codes * width}, V) for scores ({codes}, {width}), got {tuple(logits.shape)}')
    ticks = plan.shape[-2]
    npl, plan = note_plan(plan, codes, ticks, vocab)
    parents = torch.empty(codes, width, device=logits.device, dtype=torch.int32)
    notes = torch.empty(codes, width, device=logits.device, dtype=torch.int64)
    out = torch.empty(codes, width, device=logits.device, dtype=torch.float32)
    _lib.check(lib.arvae_beam_select_planned(_ptr(logits), _ptr(scores), codes, width, vocab, int(live), ctypes.byref(npl), ticks, int(tick),
                                             _ptr(parents), _ptr(notes), _ptr(out), _stream()), 'beam_select_planned')
    return parents, notes, out


def _groups_plan(plan, rows, ticks, vocab):
    """note_plan, and a uniform mask uint8 (vocab,) as the plan with both strides 0 (the grouped searches take every mask as a plan)"""
    if plan.dim() == 1:
        if plan.dtype != torch.uint8 or tuple(plan.shape) != (vocab,):
            raise ValueError(f'a uniform allowed-note mask must be uint8 of shape ({vocab},), got {plan.dtype} {tuple(plan.shape)}')
        _dev(plan)
        plan = plan.contiguous()
        return _lib.NotePlan(_ptr(plan), 0, 0), plan
    return note_plan(plan, rows, ticks, vocab)


def tick_beam_search_groups_supported(hidden, vocab, width, groups):
    """True when the one-launch diverse beam search is offered for (hidden, vocab, width, groups); else go tick by tick
    (beam_select_groups)."""
    return bool(_lib.load().arvae_tick_beam_search_groups_supported(int(hidden), int(vocab), int(width), int(groups)))


def tick_beam_search_groups(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, width, groups, penalty, plan):
    """tick_beam_search_planned in `groups` groups of width / groups beams, a group paying `penalty` per earlier-group beam that took
    the same note at the tick (arvae_tick_beam_search_groups; include/arvae_hip.h, "Diverse beam search") -> the planned call's five
    tensors, group-major, and log_probs (B, W).  plan: uint8 (B, T, V), (T, V) or one mask (V,) on the device."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    ticks, dev = beats * ticks_per_beat, gib.device
    npl, plan = _groups_plan(plan, batch, ticks, vocab)
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    parents = torch.empty(batch, ticks, width, device=dev, dtype=torch.int32)
    tokens = torch.empty(batch, ticks, width, device=dev, dtype=torch.int64)
    hist = torch.empty(batch, ticks, width, device=dev, dtype=torch.float32)
    seqs = torch.empty(batch, width, ticks, device=dev, dtype=torch.int64)
    scores = torch.empty(batch, width, device=dev, dtype=torch.float32)
    logp = torch.empty(batch, width, device=dev, dtype=torch.float32)
    ws = torch.empty(lib.arvae_tick_beam_search_ws_floats(hid), device=dev, dtype=torch.float32)
    with _timed('tick_beam_search_groups', 2.0 * batch * width * ticks * (9 * hid * hid + vocab * hid), 0.0):
        _lib.check(lib.arvae_tick_beam_search_groups(ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), batch, beats,
                                                     ticks_per_beat, hid, vocab, int(width), int(groups), float(penalty),
                                                     ctypes.byref(npl), _ptr(parents), _ptr(tokens), _ptr(hist), _ptr(seqs), _ptr(scores),
                                                     _ptr(logp), _ptr(ws), _stream()), 'tick_beam_search_groups')
    return parents, tokens, hist, seqs, scores, logp


def beam_select_groups(logits, scores, logp, live, groups, penalty, plan, tick, ticks=None):
    """beam_select_planned in `groups` groups served in order (arvae_beam_select_groups): scores and logp (codes, W), of every group the
    first `live` beams live; plan as tick_beam_search_groups (ticks: the plan's, needed with a (V,) mask) -> (parents (codes, W) int32, notes (codes, W) int64, scores (codes, W), logp (codes, W))."""
    _dev(logits, scores, logp)
    lib = _lib.load()
    logits, scores, logp = logits.contiguous(), scores.contiguous(), logp.contiguous()
    codes, width = scores.shape
    vocab = logits.shape[1]
    if (logits.shape[0] != codes * width or scores.dtype != torch.float32 or logits.dtype != torch.float32 or logp.dtype != torch.float32
            or tuple(logp.shape) != (codes, width)):
        raise ValueError(f'beam_select_groups takes float32 logits ({codes * width}, V) for scores and logp ({codes}, {width}), got '
                         f'{tuple(logits.shape)} and {tuple(logp.shape)}')
    if ticks is None and plan.dim() == 1:
        raise ValueError('beam_select_groups with one mask (V,) needs `ticks`, the number of ticks the search runs over')
    ticks = int(ticks) if ticks is not None else plan.shape[-2]
    npl, plan = _groups_plan(plan, codes, ticks, vocab)
    parents = torch.empty(codes, width, device=logits.device, dtype=torch.int32)
    notes = torch.empty(codes, width, device=logits.device, dtype=torch.int64)
    out = torch.empty(codes, width, device=logits.device, dtype=torch.float32)
    lp = torch.empty(codes, width, device=logits.device, dtype=torch.float32)
    _lib.check(lib.arvae_beam_select_groups(_ptr(logits), _ptr(scores), _ptr(logp), codes, width, int(groups), float(penalty), vocab,
                                            int(live), ctypes.byref(npl), ticks, int(tick), _ptr(parents), _ptr(notes), _ptr(out),
                                            _ptr(lp), _stream()), 'beam_select_groups')
    return parents, notes, out, lp


def sequence_log_prob_planned(weights, tokens, plan):
    """sequence_log_prob with the softmax of row r at tick t over the notes of plan[r, t] (arvae_sequence_log_prob_planned)."""
    _dev(weights, tokens)
    lib = _lib.load()
    if weights.dim() != 3 or tuple(tokens.shape) != tuple(weights.shape[:2]) or tokens.dtype != torch.int64 or weights.dtype != torch.float32:
        raise ValueError(f'sequence_log_prob takes float32 weights (R, T, V) and int64 tokens (R, T), got {tuple(weights.shape)} '
                         f'{weights.dtype} and {tuple(tokens.shape)} {tokens.dtype}')
    weights, tokens = weights.contiguous(), tokens.contiguous()
    rows, steps, vocab = weights.shape
    npl, plan = note_plan(plan, rows, steps, vocab)
    out = torch.empty(rows, device=weights.device, dtype=torch.float32)
    _lib.check(lib.arvae_sequence_log_prob_planned(_ptr(weights), _ptr(tokens), rows, steps, vocab, ctypes.byref(npl), _ptr(out), _stream()),
               'sequence_log_prob_planned')
    return out


def _sampling_uniforms(u, shape):
    if u.dtype != torch.float32 or tuple(u.shape) != tuple(shape):
        raise ValueError(f'sampling uniforms must be float32 of shape {tuple(shape)}, got {u.dtype} {tuple(u.shape)}')
    return u.contiguous()


class _EmbedFn(Function):
    @staticmethod
    def forward(ctx, idx, table, time_major):
        _dev(idx, table)
        lib = _lib.load()
        b, steps = idx.shape
        v, dim = table.shape
        rows = (steps, b) if time_major else (b, steps)
        out = torch.empty(rows + (dim,), device=table.device, dtype=torch.float32)
        _lib.check(lib.arvae_embed_fwd(_ptr(idx), _ptr(table), b, steps, dim, v, int(time_major), _ptr(out), _stream()),
                   'embed_fwd')
        ctx.save_for_backward(idx)
        ctx.table_ref, ctx.time_major = table, time_major
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        lib = _lib.load()
        table = ctx.table_ref
        b, steps = idx.shape
        v, dim = table.shape
        if table.is_leaf and table.grad is not None:
            buf, direct = _grad_target(table)                    # the parameter's own gradient buffer: add into it
        else:                                                    # (a projection table computed upstream: a fresh, overwritten tensor)
            buf, direct = torch.empty_like(table), False
        ws = torch.empty(lib.arvae_embed_bwd_ws_floats(b, steps, dim, v), device=buf.device, dtype=torch.float32)
        _lib.check(lib.arvae_embed_bwd(_ptr(idx), _ptr(g.contiguous()), b, steps, dim, v, int(ctx.time_major), _ptr(buf),
                                       int(direct), _ptr(ws), _stream()), 'embed_bwd')
        return None, (None if direct else buf), None


def segment_sum_fits(entries, positions):
    """Does the wide-row segment sum (csrc/sequence.hip, embed_bwd_wide_kernel) hold `entries` table rows x `positions` gradient rows
    in its 64 KB of LDS?  256 fp32 accumulators per entry and two ints per position of one of its 16 position groups: the bound
    arvae_embed_bwd (dim > 128) and arvae_tick_gi_bwd (entries = vocab + 1) refuse beyond."""
    return entries * 1024 + (positions + 15) // 16 * 8 <= 65536


def embed(idx, table, time_major=False):
    """nn.Embedding lookup of int64 idx [B, T] -> [B, T, D] (or [T, B, D] when time_major)."""
    if idx.dtype != torch.int64:
        raise TypeError('embedding indices must be int64')
    return _EmbedFn.apply(idx.contiguous(), table, bool(time_major))


class _TickInputFn(Function):
    """gi0 (ticks_per_beat, beats*batch, 3H) of the tick RNN's first layer from (embedding table, x_0, beat embeddings, W_ih0,
    b_ih0, fed-back tokens): one small product over vocab + 1 + beats*batch rows and a gather, instead of a whole-sequence GEMM
    over 24*batch rows of concatenated inputs (include/arvae_hip.h, arvae_tick_*; measurevae/decoder.py:459-505)."""

    @staticmethod
    def forward(ctx, table, x0, beat_emb, w_ih, b_ih, tokens, beats, tpb):
        _dev(table, x0, beat_emb, w_ih, b_ih, tokens)
        lib = _lib.load()
        vocab, emb = table.shape
        rows, hid = beat_emb.shape
        batch = rows // beats
        cols = w_ih.shape[0]
        n = vocab + 1 + rows
        dev = table.device
        x_small = torch.empty(n, emb + hid, device=dev, dtype=torch.float32)
        _lib.check(lib.arvae_tick_rows_fwd(_ptr(table), _ptr(x0), _ptr(beat_emb), 0, vocab, emb, hid, rows, _ptr(x_small), _stream()),
                   'tick_rows_fwd')
        link = Link.dense(emb + hid, cols)
        g_small = link_down(link, n, _operand(x_small), w_ih, None, ACT_NONE, None)
        gi = torch.empty(tpb, rows, cols, device=dev, dtype=torch.float32)
        with _timed('tick_gi_fwd'):
            _lib.check(lib.arvae_tick_gi_fwd(_ptr(g_small), _ptr(tokens), _ptr(b_ih), batch, beats, tpb, vocab, cols, _ptr(gi), _stream()),
                       'tick_gi_fwd')
        ctx.save_for_backward(x_small, tokens, w_ih)
        ctx.refs = (table, x0, w_ih, b_ih)
        ctx.geom = (vocab, emb, hid, rows, batch, beats, tpb, cols, link, n)
        return gi

    @staticmethod
    @once_differentiable
    def backward(ctx, d_gi):
        x_small, tokens, w_ih = ctx.saved_tensors
        table, x0, w_ref, b_ref = ctx.refs
        vocab, emb, hid, rows, batch, beats, tpb, cols, link, n = ctx.geom
        lib = _lib.load()
        dev = x_small.device
        d_gi = d_gi.contiguous()
        dg = torch.empty(n, cols, device=dev, dtype=torch.float32)
        ws = torch.empty(lib.arvae_tick_gi_bwd_ws_floats(vocab, cols), device=dev, dtype=torch.float32)
        with _timed('tick_gi_bwd'):
            _lib.check(lib.arvae_tick_gi_bwd(_ptr(d_gi), _ptr(tokens), batch, beats, tpb, vocab, cols, _ptr(dg), _ptr(ws), _stream()),
                       'tick_gi_bwd')
        gop = _operand(dg)
        # every tick row carries the bias once and exactly one note entry: db = the column sums of the vocab + 1 note rows of dG
        d_b = None
        if ctx.needs_input_grad[4]:
            bbuf, bdirect = _grad_target(b_ref)
            channel_sum(_operand(dg[:vocab + 1]), vocab + 1, cols, (0, 0), bbuf)
            d_b = None if bdirect else bbuf
        d_w = None
        if ctx.needs_input_grad[3]:
            buf, direct = _grad_target(w_ref)
            if not (direct and _defer_dense_wgrad(link, n, gop, (dg, x_small), x_small, buf, None)):
                link_wgrad(link, n, gop, _operand(x_small), buf, None, 0)
            d_w = None if direct else buf
        dx = link_up(link, n, gop, w_ih, None, ACT_NONE, None)
        tbuf, tdirect = _grad_target(table) if ctx.needs_input_grad[0] else (None, True)
        xbuf, xdirect = _grad_target(x0) if ctx.needs_input_grad[1] else (None, True)
        d_beat = torch.empty(rows, hid, device=dev, dtype=torch.float32)
        _lib.check(lib.arvae_tick_rows_bwd(_ptr(dx), vocab, emb, hid, rows, _ptr(tbuf), _ptr(xbuf), _ptr(d_beat), 0, _stream()),
                   'tick_rows_bwd')
        return (None if tdirect else tbuf), (None if xdirect else xbuf), d_beat, d_w, d_b, None, None, None


def tick_input_projection(table, x0, beat_emb, w_ih, b_ih, tokens, beats, ticks_per_beat):
    """-> gi0 (ticks_per_beat, beats*batch, 3H); tokens (batch, beats*ticks_per_beat) int64, beat_emb (beats*batch, H)"""
    return _TickInputFn.apply(table, x0, beat_emb.contiguous(), w_ih, b_ih, tokens.contiguous(), int(beats), int(ticks_per_beat))


def row_argmax(w):
    """top-1 index per row of a [rows, cols] tensor, lowest index on ties; int64 [rows]."""
    _dev(w)
    lib = _lib.load()
    w = w.contiguous()
    idx = torch.empty(w.shape[0], device=w.device, dtype=torch.int64)
    _lib.check(lib.arvae_row_argmax(_ptr(w), w.shape[0], w.shape[1], _ptr(idx), _stream()), 'row_argmax')
    return idx


def row_sample(w, u, temperature=1.0):
    """one index per row of a [rows, cols] tensor of logits, drawn from softmax(w / temperature) by inverting its CDF at u [rows] in
    (0, 1] (the decoder's multinomial feedback, measurevae/decoder.py:502-505, with the draw an explicit input); int64 [rows]."""
    _dev(w, u)
    lib = _lib.load()
    w = w.contiguous()
    u = _sampling_uniforms(u, (w.shape[0],))
    idx = torch.empty(w.shape[0], device=w.device, dtype=torch.int64)
    _lib.check(lib.arvae_row_sample(_ptr(w), w.shape[0], w.shape[1], _ptr(u), 1.0 / float(temperature), _ptr(idx), _stream()),
               'row_sample')
    return idx


def row_sample_filtered(w, u, temperature=1.0, top_k=None, top_p=None, allow=None):
    """row_sample over the notes a top-k cut, a nucleus cut and a note mask leave (arvae_row_sample_filtered; the semantics:
    include/arvae_hip.h, arvae_sample_filter_t): top_k None or 0 = off, top_p None or 1 = off, allow None or uint8 (cols,)."""
    _dev(w, u)
    lib = _lib.load()
    w = w.contiguous()
    u = _sampling_uniforms(u, (w.shape[0],))
    flt, allow = sample_filter(w.shape[1], top_k, top_p, allow)
    idx = torch.empty(w.shape[0], device=w.device, dtype=torch.int64)
    _lib.check(lib.arvae_row_sample_filtered(_ptr(w), w.shape[0], w.shape[1], _ptr(u), 1.0 / float(temperature), ctypes.byref(flt),
                                             _ptr(idx), _stream()), 'row_sample_filtered')
    return idx


class _ConcatFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        _dev(a, b)
        lib = _lib.load()
        rows, ca, cb = a.shape[0], a.shape[1], b.shape[1]
        out = torch.empty(rows, ca + cb, device=a.device, dtype=torch.float32)
        _lib.check(lib.arvae_concat_cols(_ptr(a), _ptr(b), rows, ca, cb, _ptr(out), _stream()), 'concat_cols')
        ctx.dims = (rows, ca, cb)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        rows, ca, cb = ctx.dims
        g = g.contiguous()
        da = torch.empty(rows, ca, device=g.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        db = torch.empty(rows, cb, device=g.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        _lib.check(lib.arvae_split_cols(_ptr(g), rows, ca, cb, _ptr(da), _ptr(db), 0, _stream()), 'split_cols')
        return da, db


def concat_cols(a, b):
    """torch.cat((a, b), dim=1) for 2-D tensors."""
    return _ConcatFn.apply(a.contiguous(), b.contiguous())


class _SplitFn(Function):
    @staticmethod
    def forward(ctx, x, ca):
        _dev(x)
        lib = _lib.load()
        rows, c = x.shape
        cb = c - ca
        a = torch.empty(rows, ca, device=x.device, dtype=torch.float32)
        b = torch.empty(rows, cb, device=x.device, dtype=torch.float32)
        _lib.check(lib.arvae_split_cols(_ptr(x), rows, ca, cb, _ptr(a), _ptr(b), 0, _stream()), 'split_cols')
        ctx.dims = (rows, ca, cb)
        return a, b

    @staticmethod
    @once_differentiable
    def backward(ctx, ga, gb):
        lib = _lib.load()
        rows, ca, cb = ctx.dims
        dev = (ga if ga is not None else gb).device
        ga = torch.zeros(rows, ca, device=dev) if ga is None else ga.contiguous()
        gb = torch.zeros(rows, cb, device=dev) if gb is None else gb.contiguous()
        out = torch.empty(rows, ca + cb, device=dev, dtype=torch.float32)
        _lib.check(lib.arvae_concat_cols(_ptr(ga), _ptr(gb), rows, ca, cb, _ptr(out), _stream()), 'concat_cols')
        return out, None


def split_cols(x, ca):
    """(x[:, :ca], x[:, ca:]) as contiguous tensors."""
    return _SplitFn.apply(x.contiguous(), int(ca))


class _ScaleMaskFn(Function):
    @staticmethod
    def forward(ctx, x, mask, alpha):
        _dev(x, mask)
        lib = _lib.load()
        y = torch.empty_like(x)
        _lib.check(lib.arvae_scale_mask(_ptr(x), _ptr(mask), alpha, x.numel(), 0, _ptr(y), _stream()), 'scale_mask')
        ctx.save_for_backward(mask)
        ctx.alpha = alpha
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        lib = _lib.load()
        g = g.contiguous()
        dx = torch.empty_like(g)
        _lib.check(lib.arvae_scale_mask(_ptr(g), _ptr(mask), ctx.alpha, g.numel(), 0, _ptr(dx), _stream()), 'scale_mask')
        return dx, None, None


# ------------------------------------------------------------------------------------------------
# debug-mode failure checks (ARVAE_CHECK=1): the reference's NaN-weight scan and note-index range check
# ------------------------------------------------------------------------------------------------
def checks_enabled():
    return os.environ.get('ARVAE_CHECK', '0') == '1'


def check_finite(params, what):
    """raise ValueError when any tensor of `params` holds a NaN / infinity (measurevae/encoder.py:101-106, decoder.py:420-425):
    one counting launch per tensor into one device word, ONE host sync (the reference syncs once per parameter)."""
    params = [p for p in params if p is not None and p.numel() > 0]
    if not params or torch.cuda.is_current_stream_capturing():
        return
    lib = _lib.load()
    flag = torch.zeros(1, dtype=torch.int32, device=params[0].device)
    for p in params:
        t = p.detach().contiguous()
        _dev(t)
        _lib.check(lib.arvae_count_nonfinite(_ptr(t), t.numel(), _ptr(flag), _stream()), 'count_nonfinite')
    bad = int(flag)
    if bad:
        print(f'{what} has become nan')
        raise ValueError(f'{what}: {bad} non-finite weight value(s)')


def check_index(indices, num_notes):
    """raise ValueError unless every index is in [0, num_notes) (Decoder.check_index, measurevae/decoder.py:30-41)"""
    if torch.cuda.is_current_stream_capturing():
        return
    idx = indices.contiguous()
    _dev(idx)
    flag = torch.zeros(1, dtype=torch.int32, device=idx.device)
    _lib.check(_lib.load().arvae_count_out_of_range(_ptr(idx), idx.numel(), 0, int(num_notes), _ptr(flag), _stream()),
               'count_out_of_range')
    bad = int(flag)
    if bad:
        print('Invalid Values of Indices: ', int(idx.min()), int(idx.max()))
        raise ValueError(f'{bad} note index(es) outside [0, {num_notes})')


# ------------------------------------------------------------------------------------------------
# random draws: the library's counter-based Philox4x32-10 stream (csrc/rng.h), no torch RNG kernels
# ------------------------------------------------------------------------------------------------
class RngState:
    """Every draw of the path (eps, dropout keep-masks) is element i of the stream keyed by
    (seed, offset, step + *dev_step): seed = torch.initial_seed() salted with the data-parallel rank, so the trainers'
    torch.manual_seed(rand) (image_vae_trainer.py:103) selects the stream as it does in the reference and every rank of a
    data-parallel run draws DIFFERENT noise and keep-masks for its rows ("RNG under DP": rank 0's
    stream is the single-process one); `offset` counts the draws since the stream was last selected (`rng_reseed`, called
    where the trainers call torch.manual_seed, restarts it -- the reference's generator reset).
    Under HIP-graph replay the host numbers are frozen into the captured launches, so graphed.GraphedStep advances the device
    word `dev_step` inside the graph and every replay sees fresh values."""
    offset = 0
    rank = 0                           # data-parallel rank (parallel.DataParallel sets it)
    dev_step = None                    # int32 tensor (1,) on the device, or None


RANK_SALT = 0x9E3779B97F4A7C15         # odd 64-bit constant: rank r's key = seed + r * RANK_SALT (mod 2^64)


def rng_seed():
    return (torch.initial_seed() + RngState.rank * RANK_SALT) & 0xFFFFFFFFFFFFFFFF


def rng_set_rank(rank):
    """select this process's sub-stream (0 = the single-process stream)"""
    RngState.rank = int(rank)


def rng_reseed(seed):
    """torch.manual_seed(seed) + restart of the library's stream position: what the trainers' constructors call, so that
    training seed k in a loop over seeds draws what a fresh process with --rand k draws"""
    torch.manual_seed(seed)
    RngState.offset = 0
    if RngState.dev_step is not None:
        RngState.dev_step.zero_()


def rng_next_offset():
    off = RngState.offset
    RngState.offset = (off + 1) & 0xFFFFFFFF
    return off


def rng_device_step(device, create=False):
    """the device word a captured graph advances (None until a graph asked for one)"""
    if create and (RngState.dev_step is None or RngState.dev_step.device != torch.device(device)):
        RngState.dev_step = torch.zeros(1, dtype=torch.int32, device=device)
    d = RngState.dev_step
    return d if d is not None and d.device == torch.device(device) else None


def rng_advance_device_step():
    """one more step of the device-side stream position (recorded into a graph being captured)"""
    if RngState.dev_step is not None:
        RngState.dev_step.add_(1)


def normal_noise(shape, device):
    """eps ~ N(0, 1) for z_dist.rsample() (mnist_vae.py:79, measure_vae.py:116): one library launch"""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _dev(out)
    _lib.check(_lib.load().arvae_philox_normal(_ptr(out), out.numel(), rng_seed(), rng_next_offset(), 0,
                                                _ptr(rng_device_step(device)), _stream()), 'philox_normal')
    return out


def philox_uniform(shape, device):
    """u in (0, 1], one per element, for the decoder's multinomial feedback (measurevae/decoder.py:502-505): one library launch"""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _dev(out)
    _lib.check(_lib.load().arvae_philox_uniform(_ptr(out), out.numel(), rng_seed(), rng_next_offset(), 0,
                                                 _ptr(rng_device_step(device)), _stream()), 'philox_uniform')
    return out


def keep_mask(shape, p, device):
    """uint8 keep-mask (1 with probability 1 - p) of nn.Dropout(p) / nn.GRU(dropout=p): one library launch"""
    out = torch.empty(shape, dtype=torch.uint8, device=device)
    _dev(out)
    _lib.check(_lib.load().arvae_philox_keep_mask(_ptr(out), out.numel(), 1.0 - float(p), rng_seed(), rng_next_offset(), 0,
                                                   _ptr(rng_device_step(device)), _stream()), 'philox_keep_mask')
    return out


def keep_masks(shapes, p, device):
    """the keep-masks of several Dropout layers of one step as ONE launch (arvae_philox_keep_masks); mask j is the step's next
    draw, byte for byte what keep_mask(shapes[j], ...) called in the same order would return"""
    if len(shapes) > 8:
        return [keep_mask(s, p, device) for s in shapes]
    outs = [torch.empty(s, dtype=torch.uint8, device=device) for s in shapes]
    _dev(*outs)
    n = len(outs)
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    counts = (ctypes.c_int64 * n)(*[o.numel() for o in outs])
    offsets = (ctypes.c_uint32 * n)(*[rng_next_offset() for _ in outs])
    _lib.check(_lib.load().arvae_philox_keep_masks(n, ptrs, counts, 1.0 - float(p), rng_seed(), offsets, 0, _ptr(rng_device_step(device)),
                                                   _stream()), 'philox_keep_masks')
    return outs


def dropout_mask(x, mask, p=0.5):
    """y = x * mask / (1 - p) for an explicit uint8 keep-mask (None: identity)."""
    if mask is None:
        return x
    return _ScaleMaskFn.apply(x.contiguous(), mask.contiguous(), 1.0 / (1.0 - p))


class _BroadcastFn(Function):
    @staticmethod
    def forward(ctx, v, rows):
        _dev(v)
        lib = _lib.load()
        cols = v.numel()
        y = torch.empty(rows, cols, device=v.device, dtype=torch.float32)
        _lib.check(lib.arvae_broadcast_rows(_ptr(v), rows, cols, _ptr(y), _stream()), 'broadcast_rows')
        ctx.v_ref, ctx.dims = v, (rows, cols)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rows, cols = ctx.dims
        buf, direct = _grad_target(ctx.v_ref)
        channel_sum(_operand(g.contiguous()), rows, cols, (0, 0), buf.view(-1))
        return (None if direct else buf), None


def broadcast_rows(v, rows):
    """v[None, :].expand(rows, -1) materialised (the learned start vectors)."""
    return _BroadcastFn.apply(v, int(rows))


def gather_rows_u8(src, idx, scale=1.0):
    """src (N, ...) uint8 on the device, idx (B,) int64 -> (B, ...) fp32 = scale * src[idx]."""
    _dev(src, idx)
    if src.dtype != torch.uint8 or idx.dtype != torch.int64:
        raise TypeError('gather_rows_u8 needs a uint8 source and int64 indices')
    lib = _lib.load()
    src, idx = src.contiguous(), idx.contiguous()
    row = src[0].numel()
    out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32)
    _lib.check(lib.arvae_gather_rows_u8(_ptr(src), src.shape[0], row, _ptr(idx), idx.numel(), float(scale), _ptr(out),
                                        _stream()), 'gather_rows_u8')
    return out


RENDER_SRC_LOGITS, RENDER_ROUND, RENDER_RGB = 1, 2, 4


def render_geometry(h, w, cells_per_frame, nrow, padding):
    """(Hg, Wg) of torchvision.utils.make_grid for cells_per_frame images of h x w"""
    xmaps = min(nrow, cells_per_frame)
    ymaps = -(-cells_per_frame // xmaps)
    return ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def render_frames(src, cells, nrow=8, padding=2, pad_value=1.0, logits=True, rounding=False, rgb=True, out=None):
    """Image grids as bytes, one launch for all frames (arvae_render_frames): sigmoid (logits=True), make_grid and the cast to
    uint8 of the reference's figure code.
    src (N, H, W) or (N, 1, H, W) fp32 on the device; cells (F, cells_per_frame) CPU integers, the source image of every cell of every
    frame, -1 = a blank cell -> (F, Hg, Wg, 3 if rgb else 1) uint8, what PIL.Image.fromarray takes.  rounding: floor(255 v + 0.5)
    (torchvision's save_image) instead of truncation (the .byte() of the GIF code).  One cell in one frame is rendered without
    padding, as make_grid returns a lone image.  out: a contiguous uint8 tensor of the result's size to write into."""
    import numpy as np
    if not torch.is_tensor(src) or src.dtype != torch.float32:
        raise TypeError('render_frames needs an fp32 tensor of images')
    if src.dim() == 4 and src.shape[1] == 1:
        src = src[:, 0]
    if src.dim() != 3 or src.numel() == 0:
        raise ValueError(f'render_frames needs (N, H, W) or (N, 1, H, W) images, got {tuple(src.shape)}')
    cells = np.asarray(cells.cpu() if torch.is_tensor(cells) else cells)
    if cells.ndim != 2 or cells.size == 0 or not np.issubdtype(cells.dtype, np.integer):
        raise ValueError('render_frames needs cells as a non-empty (frames, cells_per_frame) integer array')
    n, h, w = src.shape
    if cells.min() < -1 or cells.max() >= n:
        raise ValueError(f'render_frames: cells must lie in [-1, {n}) (-1 = blank), got [{cells.min()}, {cells.max()}]')
    _dev(src)
    frames, per_frame = cells.shape
    nrow, padding = int(nrow), 0 if frames == 1 and per_frame == 1 else int(padding)
    channels = 3 if rgb else 1
    lib = _lib.load()
    if lib.arvae_render_frame_bytes(h, w, per_frame, nrow, padding, channels) < 0:
        _lib.check(-1, 'render_frame_bytes')
    hg, wg = render_geometry(h, w, per_frame, nrow, padding)
    if out is None:
        out = torch.empty((frames, hg, wg, channels), device=src.device, dtype=torch.uint8)
    else:
        _dev(out)
        if out.dtype != torch.uint8 or out.numel() != frames * hg * wg * channels or out.device != src.device:
            raise ValueError(f'render_frames: out must hold {frames} x {hg} x {wg} x {channels} bytes on {src.device}')
    cells_dev = torch.from_numpy(np.ascontiguousarray(cells, dtype=np.int32)).to(src.device)
    flags = (RENDER_SRC_LOGITS if logits else 0) | (RENDER_ROUND if rounding else 0) | (RENDER_RGB if rgb else 0)
    _lib.check(lib.arvae_render_frames(_ptr(src), n, h, w, _ptr(cells_dev), frames, per_frame, nrow, padding, float(pad_value),
                                       flags, _ptr(out), _stream()), 'render_frames')
    return out.view(frames, hg, wg, channels)


def _note_tables(tables, slur, device):
    """(midi int32[V], is_note uint8[V], V) of build_measure_tables' result, with the slur index checked"""
    midi, is_note = tables[0], tables[1]
    v = midi.numel()
    if midi.dtype != torch.int32 or is_note.dtype != torch.uint8 or is_note.numel() != v or v == 0:
        raise TypeError('tables are (midi int32[V], is_note uint8[V], ...) as build_measure_tables returns them')
    if midi.device != device or is_note.device != device:
        raise ValueError(f'tables must live on {device}, where the measures are')
    if not 0 <= int(slur) < v:
        raise ValueError(f'slur index {slur} outside the vocabulary [0, {v})')
    return midi.contiguous(), is_note.contiguous(), v


def measure_notes(score, tables, *, slur, out=None):
    """(M, T) or (M, 1, T) int64 measures, T % 6 == 0 -> (M, T, 3) int32 note events per tick (arvae_measure_notes): the MIDI pitch
    sounding during the tick (0 = silence), the tick at which that element began (-1 inside leading slurs), and on a tick that
    begins an element its duration in twelfths of a quarter note (0 elsewhere).  tables: build_measure_tables' result; slur: the
    index of '__' in the vocabulary (required: the tables do not identify it, and it differs from dataset to dataset).  out: a contiguous int32 tensor of the result's size to write into."""
    if not torch.is_tensor(score) or score.dtype != torch.int64:
        raise TypeError('measure_notes needs an int64 tensor of vocabulary indices')
    if score.dim() == 3 and score.shape[1] == 1:
        score = score[:, 0]
    if score.dim() != 2 or score.numel() == 0 or score.shape[1] % 6:
        raise ValueError(f'measure_notes needs (M, T) measures with T a multiple of 6, got {tuple(score.shape)}')
    _dev(score)
    midi, is_note, v = _note_tables(tables, slur, score.device)
    score = score.contiguous()
    m, t = score.shape
    if out is None:
        out = torch.empty((m, t, 3), device=score.device, dtype=torch.int32)
    else:
        if out.dtype != torch.int32 or out.numel() != m * t * 3 or out.device != score.device or not out.is_contiguous():
            raise ValueError(f'measure_notes: out must hold {m} x {t} x 3 int32 on {score.device}')
    _lib.check(_lib.load().arvae_measure_notes(_ptr(score), m, t, _ptr(midi), _ptr(is_note), v, int(slur), _ptr(out), _stream()),
               'measure_notes')
    return out.view(m, t, 3)


def pianoroll_geometry(k, t, with_panel=False, pitch_lo=55, pitch_hi=84, px_per_twelfth=2, px_per_pitch=4, panel_cell=12, gap=8):
    """(H, W) of a piano-roll figure of k measures of t ticks (arvae_render_pianoroll)"""
    w = k * (t // 6) * 12 * px_per_twelfth
    return (pitch_hi - pitch_lo + 1) * px_per_pitch, w + (gap + k * panel_cell if with_panel else 0)


def render_pianoroll(score, tables, values=None, vmin=None, vmax=None, pitch_lo=55, pitch_hi=84, px_per_twelfth=2, px_per_pitch=4,
                     mark=None, panel_cell=12, gap=8, dot_radius=3, *, slur, out=None):
    """Piano-roll figures as bytes, one launch for all of them (arvae_render_pianoroll).
    score (F, K, T) int64 on the device: F figures of K measures each -> (F, H, W, 3) uint8, what PIL.Image.fromarray takes.
    H = (pitch_hi - pitch_lo + 1) px_per_pitch with row 0 at pitch_hi (55..84 is the reference's folk range, 55..90 its bach range);
    the roll is K (T / 6) 12 px_per_twelfth pixels wide.  values (F, K) fp32 on the device: a panel beside the roll with one dot per
    measure at the height of its value between vmin and vmax (default: the finite minimum and maximum of values; a non-finite
    value draws no dot).  mark: the pixel columns of an onset mark, by default 5 % of a beat, at least 1.  tables / slur as
    measure_notes.  out: a contiguous uint8 tensor of the result's size to write into."""
    if not torch.is_tensor(score) or score.dtype != torch.int64:
        raise TypeError('render_pianoroll needs an int64 tensor of vocabulary indices')
    if score.dim() != 3 or score.numel() == 0:
        raise ValueError(f'render_pianoroll needs (F, K, T) measures, got {tuple(score.shape)}')
    _dev(score)
    midi, is_note, v = _note_tables(tables, slur, score.device)
    score = score.contiguous()
    f, k, t = score.shape
    look = [int(x) for x in (pitch_lo, pitch_hi, px_per_twelfth, px_per_pitch)]
    if mark is None:
        mark = max(1, 12 * look[2] // 20)
    lo, hi = 0.0, 0.0
    if values is not None:
        if not torch.is_tensor(values) or values.dtype != torch.float32 or tuple(values.shape) != (f, k) or values.device != score.device:
            raise ValueError(f'render_pianoroll: values must be fp32 ({f}, {k}) on {score.device}')
        values = values.contiguous()
        if vmin is None or vmax is None:
            finite = values[torch.isfinite(values)]
            bounds = (float(finite.min()), float(finite.max())) if finite.numel() else (0.0, 0.0)
            lo, hi = (bounds[0] if vmin is None else float(vmin)), (bounds[1] if vmax is None else float(vmax))
        else:
            lo, hi = float(vmin), float(vmax)
    lib = _lib.load()
    if lib.arvae_render_pianoroll_bytes(k, t, *look, int(values is not None), int(panel_cell), int(gap)) < 0:
        _lib.check(-1, 'render_pianoroll_bytes')
    h, w = pianoroll_geometry(k, t, values is not None, *look, int(panel_cell), int(gap))
    if out is None:
        out = torch.empty((f, h, w, 3), device=score.device, dtype=torch.uint8)
    else:
        _dev(out)
        if out.dtype != torch.uint8 or out.numel() != f * h * w * 3 or out.device != score.device or not out.is_contiguous():
            raise ValueError(f'render_pianoroll: out must hold {f} x {h} x {w} x 3 contiguous bytes on {score.device}')
    _lib.check(lib.arvae_render_pianoroll(_ptr(score), f, k, t, _ptr(midi), _ptr(is_note), v, int(slur),
                                          None if values is None else _ptr(values), lo, hi, *look, int(mark), int(panel_cell), int(gap),
                                          int(dot_radius), _ptr(out), _stream()), 'render_pianoroll')
    return out.view(f, h, w, 3)


def measure_attributes(score, tables, rhythm_weights, rhythm_norm):
    """(B, 24) int64 measures -> (B, 4) [rhythmic complexity, pitch range, note density, contour]."""
    _dev(score)
    lib = _lib.load()
    midi, is_note, is_dens = tables
    b, steps = score.shape
    out = torch.empty(b, 4, device=score.device, dtype=torch.float32)
    _lib.check(lib.arvae_measure_attributes(_ptr(score.contiguous()), b, steps, _ptr(midi), _ptr(is_note), _ptr(is_dens),
                                            midi.numel(), _ptr(rhythm_weights), float(rhythm_norm), _ptr(out), _stream()),
               'measure_attributes')
    return out


# ------------------------------------------------------------------------------------------------
# the Morpho-MNIST digit classifier (csrc/resnet18.hip): inference only, no autograd
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ResnetConv:
    """Geometry of one convolution of the classifier (arvae_resnet18_conv_t): square maps, 3x3 pad 1 or 1x1 pad 0."""
    hin: int
    cin: int
    cout: int
    ksize: int = 3
    stride: int = 1

    @property
    def pad(self):
        return 1 if self.ksize == 3 else 0

    @property
    def hout(self):
        return (self.hin + 2 * self.pad - self.ksize) // self.stride + 1

    def desc(self):
        return _lib.ResnetConvDesc(self.hin, self.hin, self.cin, self.hout, self.hout, self.cout, self.ksize, self.stride, self.pad, 0)

    def label(self):
        return f'resnet18_conv<{self.hin}->{self.hout},{self.cin}->{self.cout},k{self.ksize}s{self.stride}>'


def resnet18_live_taps(geom: ResnetConv):
    """indices ky * ksize + kx of the taps that read a pixel inside the input for some output pixel (host only)"""
    taps = (ctypes.c_int32 * 9)()
    d = geom.desc()
    n = _lib.load().arvae_resnet18_live_taps(ctypes.byref(d), taps)
    if n < 0:
        _lib.check(n, 'resnet18_live_taps')
    return [int(taps[i]) for i in range(n)]


def _bn_ptrs(bn):
    if bn is None:
        return (None,) * 4
    _dev(*bn)
    return tuple(_ptr(t) for t in bn)


def resnet18_conv_prepare(geom: ResnetConv, weight, bn=None):
    """the convolution's operand planes and folded bias; bn = (weight, bias, running_mean, running_var) or None"""
    _dev(weight)
    if tuple(weight.shape) != (geom.cout, geom.cin, geom.ksize, geom.ksize):
        raise ValueError(f'weight {tuple(weight.shape)} does not match {geom}')
    lib = _lib.load()
    d = geom.desc()
    n = lib.arvae_resnet18_conv_prep_floats(ctypes.byref(d))
    if n < 0:
        _lib.check(n, 'resnet18_conv_prep_floats')
    prep = torch.empty(n, device=weight.device, dtype=torch.float32)
    _lib.check(lib.arvae_resnet18_conv_prepare(ctypes.byref(d), _ptr(weight), *_bn_ptrs(bn), _ptr(prep), _stream()),
               'resnet18_conv_prepare')
    return prep


def resnet18_conv(geom: ResnetConv, prep, x, residual=None, relu=False):
    """x (n, hin, hin, cin) NHWC -> (n, hout, hout, cout): conv + folded bias [+ residual] [ReLU]"""
    _dev(prep, x, residual)
    n = x.shape[0]
    if tuple(x.shape) != (n, geom.hin, geom.hin, geom.cin):
        raise ValueError(f'input {tuple(x.shape)} does not match {geom}')
    out = torch.empty(n, geom.hout, geom.hout, geom.cout, device=x.device, dtype=torch.float32)
    if residual is not None and tuple(residual.shape) != tuple(out.shape):
        raise ValueError(f'residual {tuple(residual.shape)} does not match the output {tuple(out.shape)}')
    d = geom.desc()
    taps = len(resnet18_live_taps(geom)) if _PROFILE is not None else 0
    with _timed(geom.label(), 2.0 * n * geom.hout * geom.hout * geom.cout * geom.cin * taps, 0.0):
        _lib.check(_lib.load().arvae_resnet18_conv(ctypes.byref(d), _ptr(prep), _ptr(x), n, _ptr(residual), int(bool(relu)), _ptr(out),
                                                   _stream()), 'resnet18_conv')
    return out


def resnet18_stem_prepare(weight, bn=None):
    _dev(weight)
    if tuple(weight.shape) != (64, 1, 7, 7):
        raise ValueError(f'stem weight {tuple(weight.shape)}, expected (64, 1, 7, 7)')
    lib = _lib.load()
    prep = torch.empty(lib.arvae_resnet18_stem_prep_floats(), device=weight.device, dtype=torch.float32)
    _lib.check(lib.arvae_resnet18_stem_prepare(_ptr(weight), *_bn_ptrs(bn), _ptr(prep), _stream()), 'resnet18_stem_prepare')
    return prep


def resnet18_stem(prep, x, relu=True):
    """x (n, 1, 28, 28) -> (n, 14, 14, 64) NHWC"""
    _dev(prep, x)
    n = x.shape[0]
    if tuple(x.shape) != (n, 1, 28, 28):
        raise ValueError(f'the classifier takes (B, 1, 28, 28) images, got {tuple(x.shape)}')
    out = torch.empty(n, 14, 14, 64, device=x.device, dtype=torch.float32)
    with _timed('resnet18_stem', 2.0 * n * 14 * 14 * 64 * 49, 0.0):
        _lib.check(_lib.load().arvae_resnet18_stem(_ptr(prep), _ptr(x), n, int(bool(relu)), _ptr(out), _stream()), 'resnet18_stem')
    return out


def resnet18_maxpool(x):
    """max-pool 3x3 stride 2 pad 1 of an NHWC tensor (padding = -inf)"""
    _dev(x)
    n, h, w, c = x.shape
    out = torch.empty(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, device=x.device, dtype=torch.float32)
    with _timed('resnet18_maxpool'):
        _lib.check(_lib.load().arvae_resnet18_maxpool(_ptr(x), n, h, w, c, _ptr(out), _stream()), 'resnet18_maxpool')
    return out


def resnet18_head(fc_w, fc_b, feat):
    """feat (n, 512) -> (logits (n, 10), softmax probabilities (n, 10), argmax (n,) int64)"""
    _dev(fc_w, fc_b, feat)
    n = feat.shape[0]
    if tuple(feat.shape) != (n, 512) or tuple(fc_w.shape) != (10, 512) or tuple(fc_b.shape) != (10,):
        raise ValueError('resnet18_head: feat (n, 512), fc_w (10, 512), fc_b (10,)')
    logits = torch.empty(n, 10, device=feat.device, dtype=torch.float32)
    probs = torch.empty_like(logits)
    pred = torch.empty(n, device=feat.device, dtype=torch.int64)
    with _timed('resnet18_head', 2.0 * n * 512 * 10, 0.0):
        _lib.check(_lib.load().arvae_resnet18_head(_ptr(fc_w), _ptr(fc_b), _ptr(feat), n, _ptr(logits), _ptr(probs), _ptr(pred), _stream()),
                   'resnet18_head')
    return logits, probs, pred


def resnet18_prepare(weights, device):
    """weights: a filled _lib.ResnetWeights over device tensors the caller keeps alive -> the prepared block of the whole network"""
    lib = _lib.load()
    prep = torch.empty(lib.arvae_resnet18_prep_floats(), device=device, dtype=torch.float32)
    _lib.check(lib.arvae_resnet18_prepare(ctypes.byref(weights), _ptr(prep), _stream()), 'resnet18_prepare')
    return prep


RESNET18_FLOP_PER_IMAGE = 2.0 * (196 * 64 * 49 + 4 * 49 * 64 * 64 * 9 + 16 * 64 * 128 * (9 + 1) + 3 * 16 * 128 * 128 * 9 +
                                 4 * 128 * 256 * (9 + 1) + 3 * 4 * 256 * 256 * 9 + 256 * 512 * (9 + 1) + 3 * 512 * 512 * 9 + 512 * 10)


def resnet18_forward(prep, x):
    """x (n, 1, 28, 28) -> (logits (n, 10), softmax probabilities (n, 10), argmax (n,) int64) in 22 launches"""
    _dev(prep, x)
    n = x.shape[0]
    if tuple(x.shape) != (n, 1, 28, 28):
        raise ValueError(f'the classifier takes (B, 1, 28, 28) images, got {tuple(x.shape)}')
    lib = _lib.load()
    size = lib.arvae_resnet18_ws_floats(n)
    if size < 0:
        _lib.check(size, 'resnet18_ws_floats')
    ws = torch.empty(size, device=x.device, dtype=torch.float32)
    logits = torch.empty(n, 10, device=x.device, dtype=torch.float32)
    probs = torch.empty_like(logits)
    pred = torch.empty(n, device=x.device, dtype=torch.int64)
    with _timed('resnet18_forward', RESNET18_FLOP_PER_IMAGE * n, 0.0):       # (the reference network's FLOP: every tap counted)
        _lib.check(lib.arvae_resnet18_forward(_ptr(prep), _ptr(x), n, _ptr(logits), _ptr(probs), _ptr(pred), _ptr(ws), _stream()),
                   'resnet18_forward')
    return logits, probs, pred


# ------------------------------------------------------------------------------------------------
# scatter figures of the latent plane (csrc/scatter.hip)
# ------------------------------------------------------------------------------------------------
SCATTER_FONT = '0123456789-.: dimenso'                 # the glyphs of csrc/scatter.hip's font, a glyph's number its place here
SCATTER_TICK_X, SCATTER_TICK_Y = 21, 22                # the two tick marks (ARVAE_SCATTER_TICK_X / _Y)
SCATTER_LABEL_CHARS = 6                                # a tick's label of more characters is left out: the margins hold six
ScatterGeometry = NamedTuple('ScatterGeometry', [(k, int) for k in ('plot_x', 'plot_y', 'plot_w', 'plot_h', 'bar_x', 'bar_w')])


def scatter_geometry(width=485, height=360, radius=2):
    """Where arvae_render_scatter puts things on a canvas of width x height: the plot area's first pixel (plot_x, plot_y) and its
    extent plot_w x plot_h, and the colour bar's first column bar_x and width bar_w (its rows are the plot area's).  Each of the
    two has a frame one pixel wide around it.  Raises for a canvas too small for the margins."""
    g = (ctypes.c_int32 * 6)()
    if _lib.load().arvae_render_scatter_bytes(int(width), int(height), int(radius), g) < 0:
        _lib.check(-1, 'render_scatter_bytes')
    return ScatterGeometry(*g)


def scatter_ticks(lo, hi, most=6):
    """[(value, label)] of an axis from lo to hi: the multiples of the smallest step among 1, 2, 5 x 10^k that leaves at most
    most + 1 of them, written with as many decimals as the step has; lo == hi gives that one value with two decimals"""
    import math
    lo, hi = float(lo), float(hi)
    if lo == hi:
        return [(lo, f'{lo:.2f}')]
    raw = (hi - lo) / most
    k = math.floor(math.log10(raw))
    for m in (1, 2, 5, 10):
        step = m * 10.0 ** k
        if step >= raw:
            break
    decimals = max(0, -(k + (1 if m == 10 else 0)))
    ticks = []
    for i in range(math.ceil(lo / step - 1e-9), math.floor(hi / step + 1e-9) + 1):
        label = f'{i * step:.{decimals}f}'
        ticks.append((i * step, label.lstrip('-') if float(label) == 0 else label))
    return ticks


def _scatter_tick_pixel(t, lo, hi, extent):
    """the pixel 0..extent - 1 of an axis of `extent` pixels at which the value t lies (the middle one when lo == hi)"""
    import math
    if lo == hi:
        return (extent - 1) // 2
    return min(extent - 1, max(0, int(math.floor((t - lo) / (hi - lo) * (extent - 1) + 0.5))))


def scatter_marks(geometry, xlim, ylim, vlim, labels):
    """The marks of one figure, a set of (x, y, glyph, rot) as arvae_scatter_mark_t holds them: tick marks and their labels on both
    axes and on the colour bar (whose values run from vlim[0] at the bottom to vlim[1] at the top), the x-axis title labels[0]
    centred below the plot and the y-axis title labels[1] turned a quarter to the left beside it.  Blanks take no mark."""
    g = geometry
    marks = set()

    def text(s, x, y, rot=0):
        for i, ch in enumerate(s):
            if ch not in SCATTER_FONT:
                raise ValueError(f'render_scatter: {ch!r} of {s!r} is not in the font {SCATTER_FONT!r}')
            if ch != ' ':
                marks.add((x, y - 6 * i - 4, SCATTER_FONT.index(ch), 1) if rot else (x + 6 * i, y, SCATTER_FONT.index(ch), 0))

    for t, label in scatter_ticks(*xlim):
        cx = g.plot_x + _scatter_tick_pixel(t, xlim[0], xlim[1], g.plot_w)
        marks.add((cx, g.plot_y + g.plot_h + 1, SCATTER_TICK_X, 0))
        if len(label) <= SCATTER_LABEL_CHARS:
            text(label, cx - (6 * len(label) - 1) // 2, g.plot_y + g.plot_h + 7)
    for lim, tick_x, right in ((ylim, g.plot_x - 5, False), (vlim, g.bar_x + g.bar_w + 1, True)):
        for t, label in scatter_ticks(*lim):
            cy = g.plot_y + g.plot_h - 1 - _scatter_tick_pixel(t, lim[0], lim[1], g.plot_h)
            marks.add((tick_x, cy, SCATTER_TICK_Y, 0))
            if len(label) <= SCATTER_LABEL_CHARS:
                text(label, tick_x + 6 if right else tick_x - 2 - (6 * len(label) - 1), cy - 3)
    text(labels[0], g.plot_x + g.plot_w // 2 - (6 * len(labels[0]) - 1) // 2, g.plot_y + g.plot_h + 18)
    text(labels[1], 3, g.plot_y + g.plot_h // 2 + (6 * len(labels[1]) - 1) // 2, rot=1)
    return marks


def _per_figure(what, given, f, width):
    """`given` as an (f, width) float32 array: one row for all figures, or one a figure"""
    import numpy as np
    a = np.asarray(given.detach().cpu() if torch.is_tensor(given) else given, dtype=np.float32)
    if width == 1 and a.shape == (f,):
        a = a.reshape(f, 1)
    elif a.shape == (width,) or (width == 1 and a.shape == ()):
        a = np.broadcast_to(a.reshape(1, width), (f, width))
    if a.shape != (f, width):
        raise ValueError(f'render_scatter: {what} is one {"value" if width == 1 else "(lo, hi) pair"} or {f} of them, got shape {a.shape}')
    return np.ascontiguousarray(a)


def render_scatter(points, values, xlim, ylim, vmin=None, vmax=None, *, width=485, height=360, radius=2, alpha=0.5,
                   labels=('dimension: 0', 'dimension: 1'), out=None):
    """Scatter figures as bytes, one launch for all of them (arvae_render_scatter): the matplotlib scatter of the reference's
    plot_dim (utils/plotting.py:41-63) in this library's own look.
    points (F, N, 2) and values (F, N) fp32 on the device: F figures (at most 16) of N points -> (F, height, width, 3) uint8, what
    PIL.Image.fromarray takes.  xlim / ylim: a (lo, hi) pair for all figures or one a figure.  vmin / vmax: a number or one a
    figure; by default the finite minimum and maximum of each figure's values (one host read; 0 and 0 where none is finite).
    A point is a filled disc of `radius` pixels in the viridis colour of its value, composited over what lies below with `alpha`
    in the order of the input (the later point on top) and clipped at the frame; a point whose coordinate or value is not
    finite draws nothing.  labels: the axis titles, a pair of strings or one pair a figure, in the characters of SCATTER_FONT.
    out: a contiguous uint8 tensor of the result's size to write into (any start address)."""
    import math
    import numpy as np
    if not torch.is_tensor(points) or not torch.is_tensor(values) or points.dtype != torch.float32 or values.dtype != torch.float32:
        raise TypeError('render_scatter needs fp32 tensors of points and values')
    if values.dim() != 2 or tuple(points.shape) != (values.shape[0], values.shape[1], 2):
        raise ValueError(f'render_scatter needs points (F, N, 2) and values (F, N), got {tuple(points.shape)} and {tuple(values.shape)}')
    f, n = values.shape
    if not 1 <= f <= _lib.SCATTER_MAX_FIGURES:
        raise ValueError(f'render_scatter renders 1 to {_lib.SCATTER_MAX_FIGURES} figures a launch, got {f}')
    limits = np.zeros((f, 6), np.float32)
    limits[:, 0:2], limits[:, 2:4] = _per_figure('xlim', xlim, f, 2), _per_figure('ylim', ylim, f, 2)
    if not (np.isfinite(limits[:, :4]).all() and (limits[:, 0] < limits[:, 1]).all() and (limits[:, 2] < limits[:, 3]).all()):
        raise ValueError('render_scatter: xlim and ylim are finite (lo, hi) pairs with lo < hi')
    if int(radius) != radius or radius < 1:
        raise ValueError(f'render_scatter: radius {radius} must be a whole number of pixels >= 1')
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f'render_scatter: alpha {alpha} outside [0, 1]')
    if len(labels) == 2 and all(isinstance(s, str) for s in labels):
        labels = [tuple(labels)] * f
    if len(labels) != f or not all(len(pair) == 2 and all(isinstance(s, str) for s in pair) for pair in labels):
        raise ValueError(f'render_scatter: labels is a pair of axis titles or {f} pairs')
    _dev(points, values)
    if points.device != values.device:
        raise ValueError('render_scatter: points and values live on different devices')
    for column, given in ((4, vmin), (5, vmax)):
        if given is not None:
            limits[:, column] = _per_figure('vmin' if column == 4 else 'vmax', given, f, 1)[:, 0]
    if vmin is None or vmax is None:                     # as render_pianoroll finds its bounds: the finite values' extremes
        finite = torch.isfinite(values)
        lo = torch.where(finite, values, torch.full_like(values, math.inf)).amin(1) if n else torch.full((f,), math.inf)
        hi = torch.where(finite, values, torch.full_like(values, -math.inf)).amax(1) if n else torch.full((f,), -math.inf)
        bounds = torch.stack([lo, hi]).cpu().numpy()
        bounds[:, ~np.isfinite(bounds).all(0)] = 0.0
        if vmin is None:
            limits[:, 4] = bounds[0]
        if vmax is None:
            limits[:, 5] = bounds[1]
    if not (np.isfinite(limits[:, 4:]).all() and (limits[:, 4] <= limits[:, 5]).all()):
        raise ValueError('render_scatter: vmin and vmax are finite with vmin <= vmax')
    g = scatter_geometry(width, height, radius)
    per_figure = [scatter_marks(g, limits[i, 0:2].tolist(), limits[i, 2:4].tolist(), limits[i, 4:6].tolist(), labels[i]) for i in range(f)]
    shared = set.intersection(*per_figure)
    table = [(m, -1) for m in sorted(shared)] + [(m, i) for i in range(f) for m in sorted(per_figure[i] - shared)]
    if len(table) > _lib.SCATTER_MAX_MARKS:
        raise ValueError(f'render_scatter: the figures need {len(table)} marks (ticks and glyphs), the table holds {_lib.SCATTER_MAX_MARKS}: '
                         'render fewer figures a call')
    marks = (_lib.ScatterMark * max(len(table), 1))(*[_lib.ScatterMark(x, y, glyph, rot, fig) for (x, y, glyph, rot), fig in table])
    width, height = int(width), int(height)
    if out is None:
        out = torch.empty((f, height, width, 3), device=values.device, dtype=torch.uint8)
    else:
        _dev(out)
        if out.dtype != torch.uint8 or out.numel() != f * height * width * 3 or out.device != values.device or not out.is_contiguous():
            raise ValueError(f'render_scatter: out must hold {f} x {height} x {width} x 3 contiguous bytes on {values.device}')
    _lib.check(_lib.load().arvae_render_scatter(_ptr(points) if n else None, _ptr(values) if n else None, f, n,
                                                limits.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), width, height, int(radius),
                                                int(math.floor(alpha * 256 + 0.5)), marks, len(table), _ptr(out), _stream()),
               'render_scatter')
    return out.view(f, height, width, 3)


def tick_beam_search_wide_supported(hidden, vocab, width, groups=1):
    """True when the streamed-weights beam search (csrc/beam_wide.hip: four launches per tick inside one call) is built for (hidden,
    vocab, width, groups): hidden 256 or 512, 2 to 128 notes, widths 1 to 16, groups dividing the width (1: not grouped)"""
    return bool(_lib.load().arvae_tick_beam_search_wide_supported(int(hidden), int(vocab), int(width), int(groups)))


def tick_beam_search_wide(weights, h0_l0, h0_l1, gib, ptab, batch, beats, ticks_per_beat, width, allow=None, allowed=None, plan=None,
                          groups=None, return_logits=False):
    """the beam search of the two-layer tick decoder at hidden 256 / 512 in one call (arvae_tick_beam_search_wide, _planned, _groups):
    neither plan nor groups -> tick_beam_search's five tensors under the mask `allow`; plan -> tick_beam_search_planned's; groups =
    (G, penalty) with plan (B, T, V), (T, V) or one mask (V,) -> tick_beam_search_groups' six.  return_logits: the logits (B, T, W, V)
    every tick's selection was made from, appended."""
    _dev(*weights, h0_l0, h0_l1, gib, ptab)
    lib = _lib.load()
    hid, vocab = weights[0].shape[1], weights[6].shape[0]
    ticks, dev, width = beats * ticks_per_beat, gib.device, int(width)
    if groups is not None:
        if plan is None:
            raise ValueError('tick_beam_search_wide: groups need a plan (every note: a mask of ones)')
        npl, plan = _groups_plan(plan, batch, ticks, vocab)
    elif plan is not None:
        npl, plan = note_plan(plan, batch, ticks, vocab)
    else:
        allow, count = _beam_mask(vocab, allow) if allowed is None or allow is None else (allow.contiguous(), int(allowed))
    n_ws = lib.arvae_tick_beam_search_wide_ws_floats(batch, ticks, hid, vocab, width)
    if n_ws < 0:
        raise RuntimeError(f'tick_beam_search_wide: {batch} codes of width {width} over {ticks} ticks at hidden size {hid} and {vocab} notes')
    tw = _lib.TickWeights(*[_ptr(t) for t in weights])
    parents = torch.empty(batch, ticks, width, device=dev, dtype=torch.int32)
    tokens = torch.empty(batch, ticks, width, device=dev, dtype=torch.int64)
    hist = torch.empty(batch, ticks, width, device=dev, dtype=torch.float32)
    seqs = torch.empty(batch, width, ticks, device=dev, dtype=torch.int64)
    scores = torch.empty(batch, width, device=dev, dtype=torch.float32)
    logp = torch.empty(batch, width, device=dev, dtype=torch.float32) if groups is not None else None
    logits = torch.empty(batch, ticks, width, vocab, device=dev, dtype=torch.float32) if return_logits else None
    ws = torch.empty(int(n_ws), device=dev, dtype=torch.float32)
    head = (ctypes.byref(tw), _ptr(h0_l0), _ptr(h0_l1), 0, _ptr(gib), _ptr(ptab), batch, beats, ticks_per_beat, hid, vocab, width)
    outs = (_ptr(parents), _ptr(tokens), _ptr(hist), _ptr(seqs), _ptr(scores))
    with _timed('tick_beam_search_wide', 2.0 * batch * width * ticks * (9 * hid * hid + vocab * hid), 0.0):
        if groups is not None:
            _lib.check(lib.arvae_tick_beam_search_wide_groups(*head, int(groups[0]), float(groups[1]), ctypes.byref(npl), *outs, _ptr(logp),
                                                              _ptr(logits), _ptr(ws), _stream()), 'tick_beam_search_wide_groups')
        elif plan is not None:
            _lib.check(lib.arvae_tick_beam_search_wide_planned(*head, ctypes.byref(npl), *outs, _ptr(logits), _ptr(ws), _stream()),
                       'tick_beam_search_wide_planned')
        else:
            _lib.check(lib.arvae_tick_beam_search_wide(*head, _ptr(allow), count, *outs, _ptr(logits), _ptr(ws), _stream()),
                       'tick_beam_search_wide')
    res = (parents, tokens, hist, seqs, scores) + (() if groups is None else (logp,))
    return res + (logits,) if return_logits else res

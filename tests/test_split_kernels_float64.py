"""The split-operand MFMA kernels of the 64-channel convolutions and of the Linear layers against float64, one kernel family at
a time through the per-layer C-ABI (raw launches, linear maps only: no activation can flip sides).  Needs a real MI355X.

Bar for every output tensor (split_cases.py):  e_hip <= R * e_cpu + FLOOR  with R = 4, FLOOR = 1e-7, e_* = relative L2 distance
to the float64 result of the HIP kernel / of torch's fp32 CPU kernel on the same fp32 inputs.  test_three_term_arithmetic.py
proves on a CPU model that this bar passes any correct fp32 accumulation and fails a kernel that loses one partial product, for
every reduction length below.  Each case prints e_hip / e_cpu.

Case -> kernel (the *_fits predicates of link_gemm.hip, conv64.hip, conv64s.hip and dense.hip; confirmed once with a
kernel trace of this file):

  link_down / link_up, 4 x 4 taps, stride 1 (CONV_LINKS x n in 3, 47, 70)
    source side has 64 channels                      conv64s_kernel<MT, NT, 0>, two-term fp16 (conv64s_weight_prep_kernel,
      c64_25, c64_12p1: down (sgn +1) and up (-1)      operand_amax_kernel in front); NT = 2 for 64 outputs, 1 for 8 / 16
      c64to8_22, c64to16_21, c64to8_9p2: down (+1)
      c8to64_22, c16to64_21, c8to64_9p2: up (-1)
    source side has 8 / 16 channels                  conv_rows_x3_kernel<true>, three-term bf16 (conv64_weight_prep_kernel)
      c64to8_22, c64to16_21, c64to8_9p2: up            e.g. the 8 -> 64 up-link at 19 -> 22
      c8to64_22, c16to64_21, c8to64_9p2: down
    gradient operand (g, y, mask, act) on c64_25     conv64s_kernel<MT, 2, 1> (no mask) / <MT, 2, 2> (keep-mask)
  link_wgrad (WGRAD_CASES x bias_side 1, 2)
    c64_25, c64to8_22, c8to64_22 (lo width <= 24)    conv_wgrad_pairs_h2_kernel<.,.>, two-term fp16, the bias sums riding along
    c64_31 (lo width 28)                             conv_wgrad_rows_x3_kernel<true, true, 4>, three-term bf16 (+ channel sums)
    c64_k3 (3 x 3 taps)                              conv_wgrad_x3_kernel<true, true>, three-term bf16 (+ channel sums)
    (each followed by conv64_wgrad_reduce_kernel)
  ops.dense, activation 0: forward, data gradient, weight and bias gradient
    DENSE_LONG (rows >= 2048, no permutation)        rows_gemm_x3_kernel<...>, three-term bf16 (+ dense_split_reduce_kernel)
    DENSE_WIDE (2888 <-> 256 with the NCHW flatten)  dense_fwd_kernel / dense_dgrad_kernel / dense_wgrad_kernel, fp32 MFMA
    DENSE_SMALL (10 <-> 256, 256 <-> 512)            the same three fp32-MFMA kernels
  ops.wide_dense (DENSE_WIDE again): the products as the whole-model executor's latent block launches them (midblock.hip)
    reduction over the 2888 side (2888 -> 256 forward,   wide_gemm_x3_kernel<WideF32, WidePlanes, partial>, three-term bf16, fp32 A,
      256 -> 2888 data gradient)                           split reduction (+ dense_split_reduce_kernel)
    reduction over the 256 side                          wide_gemm_x3_kernel<WidePlanes, WidePlanes, full>, A pre-split (mid_prep_kernel)
    weight / bias gradient                               wide_wgrad_x3_kernel, the 256-wide operand pre-split
    (weights split into planes by mid_prep_kernel; read "rows x K" forward, "K x rows" for the data gradient)

Bias sums (db*) involve no split product; they are held to the same bar, but the CPU model's separation claim (reduction lengths
of split_cases.reduction_lengths()) is about the products only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from single_channel_cases import SELU_SA, fold as _fold          # (the folded gradient operand, shared with the single-channel links' test)
from split_cases import (CONV_BATCHES, CONV_LINKS, DENSE_LONG, DENSE_SMALL, DENSE_WIDE, FLOOR, R, WGRAD_CASES, link_geometry)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _rel(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def _hold(case, got, cpu, ref):
    """assert the bar on every tensor of `got` (HIP) against `ref` (float64) with `cpu` (torch fp32) as the yardstick"""
    bad = []
    for k in got:
        assert np.all(np.isfinite(got[k])), (case, k)
        e_hip, e_cpu = _rel(got[k], ref[k]), _rel(cpu[k], ref[k])
        ratio = e_hip / e_cpu if e_cpu > 0 else float('inf' if e_hip > 0 else 0)
        print(f'{case} {k}: e_hip {e_hip:.3e}  e_cpu {e_cpu:.3e}  e_hip/e_cpu {ratio:.2f}  bar {R * e_cpu + FLOOR:.3e}')
        if not e_hip <= R * e_cpu + FLOOR:
            bad.append((k, e_hip, e_cpu))
    assert not bad, (case, bad)


def _link(name):
    from arvae_amd import ops
    hi, chi, lo, clo, pad, k = link_geometry(name)
    return ops.Link(hi, hi, chi, lo, lo, clo, k, k, 1, pad)


def _tensors(name, n, seed):
    """channels-last fp32 tensors of a link: hi, lo, weights [clo][chi][k][k] (x 0.2, as CONV_CASES), the two biases"""
    hi, chi, lo, clo, _pad, k = link_geometry(name)
    rs = np.random.RandomState(seed)
    return dict(hi=rs.standard_normal((n, hi, hi, chi)).astype(np.float32), lo=rs.standard_normal((n, lo, lo, clo)).astype(np.float32),
                w=(rs.standard_normal((clo, chi, k, k)) * 0.2).astype(np.float32),
                b_lo=rs.standard_normal(clo).astype(np.float32), b_hi=rs.standard_normal(chi).astype(np.float32))


def _nchw(a, dtype):
    return (a if torch.is_tensor(a) else torch.from_numpy(a)).to(dtype).permute(0, 3, 1, 2)


def _maps_torch(name, t, dtype, hi=None, lo=None, want=('down', 'up', 'dw', 'db1', 'db2')):
    """the link's maps in torch on the CPU (float64: the reference; float32: the yardstick).  hi / lo: operands as multiplied
    (torch tensors) when they are not the plain tensors of t"""
    pad = link_geometry(name)[4]
    hi = _nchw(t['hi'] if hi is None else hi, dtype)
    lo = _nchw(t['lo'] if lo is None else lo, dtype)
    w = torch.from_numpy(t['w']).to(dtype).requires_grad_(True)
    out = {}
    if 'down' in want:
        out['down'] = F.conv2d(hi, w, torch.from_numpy(t['b_lo']).to(dtype), padding=pad).detach().permute(0, 2, 3, 1).numpy()
    if 'up' in want:
        out['up'] = F.conv_transpose2d(lo, w, torch.from_numpy(t['b_hi']).to(dtype), padding=pad).detach().permute(0, 2, 3, 1).numpy()
    if 'dw' in want:
        F.conv2d(hi, w, None, padding=pad).backward(lo)          # dW of the Conv2d for the upstream gradient `lo`
        out['dw'] = w.grad.numpy()
    if 'db1' in want:
        out['db1'] = lo.sum((0, 2, 3)).numpy()
    if 'db2' in want:
        out['db2'] = hi.sum((0, 2, 3)).numpy()
    return out


def _maps_hip(dev, name, t, n, hi_op=None, lo_op=None, want=('down', 'up', 'dw', 'db1', 'db2')):
    """the same maps through the raw launches; hi_op / lo_op: builders of a gradient operand from the device tensors"""
    from arvae_amd import ops
    link = _link(name)
    d = {k: torch.from_numpy(v).to(dev) for k, v in t.items() if isinstance(v, np.ndarray)}
    hi = ops._operand(d['hi']) if hi_op is None else ops._operand(d['hi'], d['y_hi'], d.get('m_hi'), hi_op)
    lo = ops._operand(d['lo']) if lo_op is None else ops._operand(d['lo'], d['y_lo'], d.get('m_lo'), lo_op)
    out = {}
    if 'down' in want:
        out['down'] = ops.link_down(link, n, hi, d['w'], d['b_lo'], ops.ACT_NONE, None)
    if 'up' in want:
        out['up'] = ops.link_up(link, n, lo, d['w'], d['b_hi'], ops.ACT_NONE, None)
    for side in (1, 2):
        if f'db{side}' in want:
            dw, db = torch.zeros_like(d['w']), torch.zeros_like(d['b_lo'] if side == 1 else d['b_hi'])
            ops.link_wgrad(link, n, lo, hi, dw, db, side)
            out[f'db{side}'] = db
            out[f'dw{side}'] = dw
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return out


def _with_both_dw(maps):
    """the torch maps hold one dW; the HIP side computes it once per bias side"""
    maps = dict(maps)
    dw = maps.pop('dw', None)
    if dw is not None:
        maps['dw1'] = maps['dw2'] = dw
    return maps


# ---------------------------------------------------------------- forward products of the 64-channel links
@pytest.mark.parametrize('n', CONV_BATCHES)
@pytest.mark.parametrize('name', list(CONV_LINKS))
def test_conv64_down_and_up_vs_float64(dev, name, n):
    """link_down and link_up of every link of CONV_LINKS: the row-staged two-term fp16 kernel with both signs of the tap walk,
    64 / 16 / 8 output channels, padded and not, and the three-term bf16 gathering kernel where the source side is narrow."""
    t = _tensors(name, n, 1000 * n + len(name))
    want = ('down', 'up')
    _hold(f'{name} n={n}', _maps_hip(dev, name, t, n, want=want), _maps_torch(name, t, torch.float32, want=want),
          _maps_torch(name, t, torch.float64, want=want))


# ---------------------------------------------------------------- weight / bias gradients
@pytest.mark.parametrize('name,n', WGRAD_CASES, ids=[f'{a}-n{b}' for a, b in WGRAD_CASES])
def test_conv64_wgrad_vs_float64(dev, name, n):
    """link_wgrad with bias_side 1 and 2 (dw1 / db1, dw2 / db2): 64 <-> 64, 64 <-> 8 and 8 <-> 64 on the paired-rows fp16 kernel,
    a wider and a 3 x 3 layer on the two bf16 kernels; one image, and batches whose pixel count is no multiple of anything."""
    t = _tensors(name, n, 77 * n + len(name))
    want = ('dw', 'db1', 'db2')
    _hold(f'{name} n={n}', _maps_hip(dev, name, t, n, want=want), _with_both_dw(_maps_torch(name, t, torch.float32, want=want)),
          _with_both_dw(_maps_torch(name, t, torch.float64, want=want)))


# ---------------------------------------------------------------- gradient operands with a folded activation
@pytest.mark.parametrize('hidden_max', [False, True], ids=['plain_max', 'max_removed'])
@pytest.mark.parametrize('use_mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('act', [1, 2], ids=['relu', 'selu'])
def test_folded_gradient_operands_vs_float64(dev, act, use_mask, hidden_max):
    """The operand (g, y, mask, act) on the 64 <-> 64 layer, on the lo side (link_up, link_wgrad bias_side 1) and on the hi side
    (link_down, link_wgrad bias_side 2).  Both references multiply by act'(y) * mask computed from the same fp32 y.
    max_removed: the largest |g| (10^6 x the bulk) sits where the keep-mask is zero (mask) or where y <= 0 (ReLU) or at the y of
    the smallest SELU slope, so the maximum of the operand AS MULTIPLIED (conv64_operand_amax) is not the raw maximum: a scale
    taken from raw g would push the bulk's low fp16 terms into subnormals (error ~2^-39 x 10^6 x max / rms ~ 1e-5 here)."""
    name, n = 'c64_25', 6
    plain = _tensors(name, n, 31 + act + 2 * use_mask)
    rs = np.random.RandomState(5 + act)
    got, cpu, ref = {}, {}, {}
    for side, want in (('lo', ('up', 'dw', 'db1')), ('hi', ('down', 'dw', 'db2'))):
        t = dict(plain)                                              # the other side stays a plain tensor
        shape = t[side].shape
        y = rs.standard_normal(shape).astype(np.float32)
        m = (rs.random_sample(shape) >= 0.5).astype(np.uint8) if use_mask else None
        if act == 1:
            y = np.maximum(y, 0)                                     # a saved ReLU output
        if m is not None:
            y = y * m * 2.0                                          # ... of a layer with dropout: kept values times two
        if hidden_max:
            at = (n // 2, 7, 9, 11)
            if m is not None:
                m[at], y[at] = 0, 0.0
            elif act == 1:
                y[at] = 0.0
            else:
                y[at] = -SELU_SA * (1.0 - 2.0 ** -20)                 # SELU derivative ~ 1.7e-6: the product is of the bulk's size
            t[side] = t[side].copy()
            t[side][at] = 1.0e6 * np.abs(t[side]).max()
        t[f'y_{side}'] = y.astype(np.float32)
        if m is not None:
            t[f'm_{side}'] = m
        g = _maps_hip(dev, name, t, n, want=want, **{f'{side}_op': act})
        for dtype, dst in ((torch.float32, cpu), (torch.float64, ref)):
            folded = _fold(t[side], t[f'y_{side}'], t.get(f'm_{side}'), act, dtype)
            r = _with_both_dw(_maps_torch(name, t, dtype, want=want, **{side: folded}))
            dst.update({f'{side}:{k}': v for k, v in r.items() if k in g})
        got.update({f'{side}:{k}': v for k, v in g.items()})
    _hold(f'folded act={act} mask={use_mask} hidden_max={hidden_max}', got, cpu, ref)


# ---------------------------------------------------------------- scaling and outliers of the fp16-scaled kernels
def test_conv64_scaling_is_exact_and_survives_outliers(dev):
    """test_conv32_scaling_is_exact_and_survives_outliers for the 64-channel fp16-scaled kernels (conv64s forward and backward,
    the paired-rows weight gradient).  (1) A tensor times 2^k gives bit for bit the result times 2^k.  (2) One value 10^4 times
    the bulk, in the source and in the gradient: the whole-tensor bar still holds, and the outputs the outlier does not reach
    keep their accuracy relative to THEIR norm.  Their bar comes from the two-term model (test_two_term_arithmetic.py): every
    value is reproduced to 2^-39 of the tensor's maximum, so the far outputs carry at most 2^-39 * max / rms(bulk) relative
    error from the split, on top of the ordinary bar.  (3) All-zero and 1e-38-sized sources give finite results and exact zeros."""
    name, n = 'c64_25', 4
    t = _tensors(name, n, 5)
    t['hi'] = np.maximum(t['hi'], 0)                                 # ReLU-like: half zeros
    t['b_lo'][:] = 0
    t['b_hi'][:] = 0
    want = ('down', 'up', 'dw', 'db1')
    base = _maps_hip(dev, name, t, n, want=want)
    for k_hi, k_lo, k_w in ((-23, 0, 0), (9, -30, 0), (0, 0, -7), (-12, 14, 5)):
        s_hi, s_lo, s_w = np.float32(2.0 ** k_hi), np.float32(2.0 ** k_lo), np.float32(2.0 ** k_w)
        got = _maps_hip(dev, name, dict(t, hi=t['hi'] * s_hi, lo=t['lo'] * s_lo, w=t['w'] * s_w), n, want=want)
        np.testing.assert_array_equal(got['down'], base['down'] * (s_hi * s_w))
        np.testing.assert_array_equal(got['up'], base['up'] * (s_lo * s_w))
        np.testing.assert_array_equal(got['dw1'], base['dw1'] * (s_hi * s_lo))
        np.testing.assert_array_equal(got['db1'], base['db1'] * s_lo)          # the bias sums ride in the weight-gradient kernel
    ref_plain = _maps_torch(name, t, torch.float64, want=('down', 'up'))
    # one outlier at a time, first in the source (hi), then in the gradient (lo): each run holds the whole-tensor bar on every map
    # (the weight gradient sees the outlier on one of its two operands), and the map that reads the tensor directly has a far region:
    # `down` pixel (oy, ox) reads hi rows oy .. oy + 3, `up` pixel (y, x) reads lo rows y - 3 .. y
    far_down = np.ones(base['down'].shape[:3], bool)
    far_down[1, 4:8, 6:10] = False
    far_up = np.ones(base['up'].shape[:3], bool)
    far_up[2, 5:9, 3:7] = False
    for src, at, sign, k, far in (('hi', (1, 7, 9, 11), 1.0, 'down', far_down), ('lo', (2, 5, 3, 4), -1.0, 'up', far_up)):
        out = dict(t)
        out[src] = t[src].copy()
        out[src][at] = sign * 1.0e4 * np.abs(t[src]).max()
        got = _maps_hip(dev, name, out, n, want=want)
        cpu, ref = (_with_both_dw(_maps_torch(name, out, dt, want=want)) for dt in (torch.float32, torch.float64))
        _hold(f'outlier in {src}', got, cpu, ref)
        np.testing.assert_allclose(ref[k][far], ref_plain[k][far], rtol=1e-9, atol=1e-12)          # the outlier does not reach these
        assert np.all(got[k][~far] != base[k][~far])
        e_hip, e_cpu = _rel(got[k][far], ref[k][far]), _rel(cpu[k][far], ref[k][far])
        bulk = t[src][t[src] != 0]
        bar = 2.0 ** -39 * float(np.abs(out[src]).max()) / float(np.sqrt(np.mean(bulk.astype(np.float64) ** 2))) + R * e_cpu + FLOOR
        print(f'outlier in {src}, {k} far region: e_hip {e_hip:.3e}  e_cpu {e_cpu:.3e}  bar {bar:.3e}')
        assert e_hip <= bar, (k, e_hip, bar)
    # zeros and a denormal-range maximum
    zero = dict(t, hi=np.zeros_like(t['hi']), lo=np.zeros_like(t['lo']))
    got = _maps_hip(dev, name, zero, n, want=want)
    for k in ('down', 'up', 'dw1', 'db1'):
        assert np.all(got[k] == 0), k
    tiny = dict(zero, hi=zero['hi'].copy(), lo=zero['lo'].copy())
    tiny['hi'][0, 3:6, 2:20, :] = np.float32(1e-38)
    tiny['lo'][0, 3:6, 2:20, :] = np.float32(-1e-38)
    got = _maps_hip(dev, name, tiny, n, want=want)
    for k in got:
        assert np.all(np.isfinite(got[k])), k
    assert np.all(got['down'][1:] == 0) and np.all(got['up'][1:] == 0)
    assert np.all(got['down'][0, 6:] == 0) and np.all(got['up'][0, 9:] == 0) and np.all(got['up'][0, :3] == 0)
    got = _maps_hip(dev, name, dict(tiny, lo=zero['lo']), n, want=('dw', 'db1'))
    assert np.all(got['dw1'] == 0) and np.all(got['db1'] == 0)


# ---------------------------------------------------------------- Linear layers
def _to_mem(t, perm):          # NCHW-flatten feature order -> channels-last memory order
    if perm == (0, 0):
        return t.contiguous()
    c, hw = perm
    return t.reshape(t.shape[0], c, hw).permute(0, 2, 1).reshape(t.shape[0], -1).contiguous()


def _from_mem(t, perm):
    if perm == (0, 0):
        return t
    c, hw = perm
    return t.reshape(t.shape[0], hw, c).permute(0, 2, 1).reshape(t.shape[0], -1)


def _dense_tensors(case):
    rows, fin, fout, _in_perm, _out_perm = case
    rs = np.random.RandomState(rows + fin)
    x = torch.from_numpy(rs.standard_normal((rows, fin)).astype(np.float32))            # feature order = NCHW flatten
    w = torch.from_numpy((rs.standard_normal((fout, fin)) / np.sqrt(fin)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(fout).astype(np.float32))
    gy = torch.from_numpy(rs.standard_normal((rows, fout)).astype(np.float32))
    return x, w, b, gy


def _dense_torch(x, w, b, gy, dtype, bias=True):
    xr, wr, br = (v.detach().clone().to(dtype).requires_grad_(True) for v in (x, w, b))
    y = F.linear(xr, wr, br if bias else None)
    y.backward(gy.to(dtype))
    return {'y': y.detach().numpy(), 'dx': xr.grad.numpy(), 'dw': wr.grad.numpy(),
            'db': br.grad.numpy() if bias else gy.to(dtype).sum(0).numpy()}


@pytest.mark.parametrize('case', DENSE_WIDE + DENSE_LONG + DENSE_SMALL, ids=str)
def test_dense_vs_float64(dev, case):
    """ops.dense with activation 0: forward, data gradient, weight gradient and bias gradient of nn.Linear (with the NCHW-flatten
    permutation on either side for the 2888-feature layers); rows ragged against every tile, and the headline batches."""
    from arvae_amd import ops
    rows, fin, fout, in_perm, out_perm = case
    x, w, b, gy = _dense_tensors(case)
    xd = _to_mem(x, in_perm).to(dev).requires_grad_(True)
    wd, bd = (v.to(dev).requires_grad_(True) for v in (w, b))
    yd = ops.dense(xd, wd, bd, ops.Link.dense(fin, fout, in_perm=in_perm, out_perm=out_perm), 0)
    yd.backward(_to_mem(gy, out_perm).to(dev))
    got = {'y': _from_mem(yd.detach().cpu(), out_perm).numpy(), 'dx': _from_mem(xd.grad.cpu(), in_perm).numpy(),
           'dw': wd.grad.cpu().numpy(), 'db': bd.grad.cpu().numpy()}
    _hold(f'dense {case}', got, _dense_torch(x, w, b, gy, torch.float32), _dense_torch(x, w, b, gy, torch.float64))


@pytest.mark.parametrize('case', DENSE_WIDE, ids=str)
def test_wide_tile_kernels_vs_float64(dev, case):
    """The same 2888 <-> 256 layers on the three-term bf16 tile kernels the whole-model executor's latent block runs them on
    (ops.wide_dense: wide_gemm_x3_kernel with fp32 or pre-split A, split reduction or one pass, weights read either way;
    wide_wgrad_x3_kernel with either operand pre-split), rows ragged against the 64 x 64 tile and the headline batches.  The
    product that reduces over the 2888 side is a split reduction whose consumer adds the bias: it is compared without one."""
    from arvae_amd import ops
    rows, fin, fout, in_perm, out_perm = case
    x, w, b, gy = _dense_tensors(case)
    bias = fin < fout                                    # forward over the short side: one pass with bias
    link = ops.Link.dense(fin, fout, in_perm=in_perm, out_perm=out_perm)
    xd, gd = _to_mem(x, in_perm).to(dev), _to_mem(gy, out_perm).to(dev)
    wd, bd = w.to(dev), b.to(dev)
    dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
    y = ops.wide_dense(link, rows, 0, wd, x=xd, bias=bd if bias else None)
    dx = ops.wide_dense(link, rows, 1, wd, g=gd)
    ops.wide_dense(link, rows, 2, wd, x=xd, g=gd, dw=dw, dbias=db)
    torch.cuda.synchronize()
    got = {'y': _from_mem(y.cpu(), out_perm).numpy(), 'dx': _from_mem(dx.cpu(), in_perm).numpy(), 'dw': dw.cpu().numpy(),
           'db': db.cpu().numpy()}
    _hold(f'wide {case}', got, _dense_torch(x, w, b, gy, torch.float32, bias), _dense_torch(x, w, b, gy, torch.float64, bias))

"""Case tables, float64 references, fp32 yardsticks and the bar of the float64 accuracy tests of the single-channel links: the first
encoder layer and the last decoder layer of both image models (ar-vae_amd/csrc/conv_c1.hip, wgrad_c1s.h, and the 1 <-> 64 kernels of
link_gemm.hip).  Shared by the GPU test (test_single_channel_links_float64.py) and by the CPU test that proves the references right
and the table sharp (test_single_channel_cases.py).  No test in here.

The bar: tensors    e_got <= R * e_cpu + FLOOR                                    (split_cases.py; e_* = relative L2 distance to float64)
         the single-channel bias sum, one number (key 'db2', 0-d)
                    |got - ref| <= max(R * |cpu - ref|, SCALAR_RTOL * |ref|)      (loss_cases.py)
None of these kernels splits an operand: they are fp32 MFMA or vector FMA, so the bar mostly catches indexing, border and
reduction-structure errors.

A case is a Case tuple.  The maps are linear: activation ACT_NONE, bias or none, an output keep-mask (x 2 mask) where the route takes
one, gradient operands (g, y, mask, act) folded in both dtypes from the same fp32 y (fold()).
  route 'down'   lo = conv(hi) + b_lo                      -> {'down'}
  route 'up'     hi = conv_transpose(lo) + b_hi            -> {'up'}
  route 'wgrad'  dW of the Conv2d for the upstream gradient lo, the bias sums of both sides
                                                           -> {'dw', 'db1' (sums of lo per channel), 'db2' (the sum of hi, 0-d)}
Batches that depend on the device are written 'cus+1' and resolved by batch(case, cus): cus = 256 on the MI355X, and the GPU test
passes multi_processor_count.

  inputs(case, cus)            fp32 tensors, channels-last, seeded by the case's id
  maps_torch(case, inp, dtype) reference (a): torch on the CPU, float64 the reference, float32 the yardstick
  maps_numpy(case, inp)        reference (b): numpy float64 by explicit patches, einsum over [row, position, tap]
  wgrad_stream(case, inp)      fp32 numpy restatement of the streaming weight gradients' own summation order
  WRONG_KERNELS                deliberate defects: float64 arithmetic altered, rounded once to fp32"""
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from loss_cases import SCALAR_RTOL, hold, rel                 # noqa: F401  (the 0-d rule and the tensor rule, printed and returned)
from split_cases import FLOOR, R                              # noqa: F401

f32, f64 = np.float32, np.float64
CUS = 256                                                     # compute units of the MI355X

SELU_SCALE = float(np.float32(1.0507009873554805))          # the kernels' fp32 constants (common.h), so that the float64
SELU_SA = float(np.float32(1.0507009873554805) * np.float32(1.6732632423543772))       # reference is the SAME operation


def fold(g, y, mask, act, dtype):
    """a gradient operand as multiplied (common.h Operand::at): g * act'(y) [* 2 mask, y read as y / 2], in `dtype` from fp32 data"""
    g, y = torch.from_numpy(g).to(dtype), torch.from_numpy(y).to(dtype)
    if mask is not None:
        g, y = g * (2.0 * torch.from_numpy(mask).to(dtype)), y * 0.5
    if act == 1:
        return g * (y > 0).to(dtype)
    return g * torch.where(y > 0, torch.full_like(y, SELU_SCALE), y + SELU_SA)


# ---------------------------------------------------------------------------------------------------------------- geometry, cases
Geom = namedtuple('Geom', 'hh hw lh lw clo k s p')           # hi [n, hh, hw, 1] <-> lo [n, lh, lw, clo], k x k taps, stride, pad


def geom(hh, hw, clo, k=4, s=1, p=0):
    return Geom(hh, hw, (hh + 2 * p - k) // s + 1, (hw + 2 * p - k) // s + 1, clo, k, s, p)


# route: 'down' / 'up' / 'wgrad'; n: an int or 'cus+1'; bias: forward maps with a bias; out_mask: forward maps with an output keep-mask;
# fold: None or (side 'hi' / 'lo', act 1 ReLU / 2 SELU, with a keep-mask); kernel: the kernel the case is meant to reach; why: its edge
Case = namedtuple('Case', 'route geom n bias out_mask fold kernel why repeat')


def _c(route, g, n, kernel, why, bias=True, out_mask=False, fold=None, repeat=False):
    return Case(route, g, n, bias, out_mask, fold, kernel, why, repeat)


G_DS = geom(64, 64, 32, 4, 2, 1)                              # dSprites conv1 / deconv4: 64 x 64 <-> 32 x 32 x 32
G_MN = geom(28, 28, 64)                                       # Morpho-MNIST first / last layer: 28 x 28 <-> 25 x 25 x 64
RELU_LO, RELU_HI, SELU_MASK_LO, SELU_MASK_HI = ('lo', 1, False), ('hi', 1, False), ('lo', 2, True), ('hi', 2, True)

# ---- 64 x 64 <-> 32 x 32 x 32, k4 s2 p1 (conv_c1.hip)
C1_CASES = [
    _c('down', G_DS, 1, 'down_c1s_kernel<0>', 'one image: 8 workgroups, every wave one row', bias=False),
    _c('down', G_DS, 3, 'down_c1s_kernel<0>', 'no second row anywhere'),
    _c('down', G_DS, 129, 'down_c1s_kernel<0>', '4128 rows: 32 waves get a second row, the others prefetch past the end', repeat=True),
    _c('down', G_DS, 3, 'down_c1s_kernel<0>', 'source (g, y, ReLU): the at2 path', fold=RELU_HI),
    _c('up', G_DS, 1, 'up_c1_kernel<0, false>', 'one image: two tiles', bias=False),
    _c('up', G_DS, 3, 'up_c1_kernel<0, false>', 'six tiles, one per workgroup'),
    _c('up', G_DS, 'cus+1', 'up_c1_kernel<0, false>', 'two workgroups get a second tile: both LDS buffers', repeat=True),
] + [_c('wgrad', G_DS, n, 'wgrad_c1s_kernel', why, repeat=n == 130)
     for n, why in ((1, '4 groups'), (3, '12 groups'), (64, '2048 rows: exactly full'), (65, '32 waves get a second row'),
                    (130, '4160 rows: waves with two and three rows'))] + [
    _c('wgrad', G_DS, 3, 'wgrad_c1s_kernel', 'lo = (g, y, ReLU): what autograd sends for conv1', fold=RELU_LO),
    _c('wgrad', G_DS, 65, 'wgrad_c1s_kernel', 'lo = (g, y, ReLU) with a second pass', fold=RELU_LO),
    _c('wgrad', G_DS, 3, 'wgrad_c1s_kernel', 'hi = (g, y, ReLU): the hi side folded', fold=RELU_HI),
]

# ---- 1 -> 64 down (link_gemm.hip down_single_channel_mfma_kernel)
DOWN64 = 'down_single_channel_mfma_kernel'
DOWN64_CASES = [
    _c('down', G_MN, 1, DOWN64, '<= 1024 pixels; 625 positions leave one in the last tile', bias=False),
    _c('down', G_MN, 5, DOWN64, '<= 1024 pixels; 625 positions leave one in the last tile'),
    _c('down', G_MN, 5, DOWN64, 'the keep-mask epilogue', out_mask=True),
    _c('down', G_MN, 5, DOWN64, 'the folded-operand gather', fold=SELU_MASK_HI),
    _c('down', geom(33, 33, 64), 2, DOWN64, '1089 pixels: the Operand loop with a plain operand'),
    _c('down', geom(64, 64, 64, 4, 2, 1), 2, DOWN64, 'stride 2, pad, 4096 pixels, 1024 positions'),
    _c('down', geom(14, 14, 64, 3, 1, 1), 3, DOWN64, '9 taps: the B rows of taps 9-15 are zero; padded reads'),
    _c('down', geom(10, 31, 64), 3, DOWN64, 'non-square map'),
]

# ---- 64 / 32 / other -> 1 up
UP4, UP2, UPV = 'up_single_channel_mfma_kernel<4>', 'up_single_channel_mfma_kernel<2>', 'up_single_channel_kernel'
UP_CASES = [
    _c('up', G_MN, 1, UP4, '625 positions: 40 M-tiles, the last with one position', bias=False),
    _c('up', G_MN, 4, UP4, 'four workgroups'),
    _c('up', geom(17, 17, 64), 2, UP4, '196 positions: fewer M-tiles than two rounds of the eight waves'),
    _c('up', G_MN, 4, UP4, 'the keep-mask epilogue', out_mask=True),
    _c('up', geom(32, 32, 32, 4, 2, 1), 3, UP2, 'clo 32 off the 64 x 64 geometry, stride 2'),
    _c('up', geom(15, 15, 32), 3, UP2, 'clo 32, stride 1', bias=False),
    _c('up', geom(22, 22, 16), 3, UPV, 'clo 16'),
    _c('up', geom(12, 12, 8), 2, UPV, 'clo 8', out_mask=True),
    _c('up', geom(42, 42, 64), 2, UPV, 'clo 64 with 1521 positions x 17 floats: more than 96 KB of LDS'),
]

# ---- 1 <-> 64 s1 weight gradient (conv_c1.hip wgrad_c1w_kernel)
C1W = 'wgrad_c1w_kernel'
C1W_CASES = [
    _c('wgrad', G_MN, 1, C1W, '25 rows: 4 groups, the last with one row'),
    _c('wgrad', G_MN, 5, C1W, '125 rows'),
    _c('wgrad', G_MN, 82, C1W, '2050 rows: two waves get a second row'),
    _c('wgrad', G_MN, 5, C1W, 'lo = (g, y, SELU, keep-mask)', fold=SELU_MASK_LO),
    _c('wgrad', G_MN, 5, C1W, 'hi = (g, y, ReLU)', fold=RELU_HI),
    _c('wgrad', geom(31, 31, 64), 3, C1W, 'lw = 28: every slot live, hw at its maximum'),
    _c('wgrad', geom(7, 7, 64), 3, C1W, 'lw = 4: one quad'),
    _c('wgrad', geom(4, 4, 64), 5, C1W, 'lh = lw = 1: row r and the last lo row coincide'),
    _c('wgrad', geom(10, 31, 64), 3, C1W, 'non-square'),
    _c('wgrad', geom(31, 10, 64), 3, C1W, 'non-square, transposed'),
]

# ---- one step outside each predicate: the generic kernels, held to the same bar
GENERIC = 'link_gemm_kernel'
OUTSIDE_CASES = [
    _c('down', geom(19, 19, 16), 3, GENERIC, 'down 1 -> 16: outside single_channel_mfma_fits'),
    _c('wgrad', geom(32, 32, 64), 2, GENERIC, 'lw = 29: outside conv_c1w_fits'),
    _c('up', G_DS, 3, GENERIC, 'the 64 x 64 geometry with a folded lo operand: outside the conv_c1 up route', fold=RELU_LO),
]

CASES = C1_CASES + DOWN64_CASES + UP_CASES + C1W_CASES + OUTSIDE_CASES


def batch(case, cus=CUS):
    return cus + 1 if case.n == 'cus+1' else int(case.n)


def case_id(case):
    g = case.geom
    hi = f'{g.hh}' if g.hh == g.hw else f'{g.hh}x{g.hw}'
    lo = f'{g.lh}' if g.lh == g.lw else f'{g.lh}x{g.lw}'
    tag = f'{case.route}-{hi}to{lo}c{g.clo}k{g.k}s{g.s}p{g.p}-n{case.n}'
    if not case.bias and case.route != 'wgrad':
        tag += '-nobias'
    if case.out_mask:
        tag += '-outmask'
    if case.fold is not None:
        side, act, masked = case.fold
        tag += f'-{side}_{"relu" if act == 1 else "selu"}{"_mask" if masked else ""}'
    if case.kernel == GENERIC:
        tag += '-generic'
    return tag


assert len({case_id(c) for c in CASES}) == len(CASES)

# seeds: crc32 of the id plus a salt.  A salt is set where the first seed left the single-channel bias sum (a signed sum when hi is
# a folded gradient) under a tenth of sqrt(count) x rms: test_single_channel_cases.py asserts that condition for every 0-d output
SEED_SALT = {}


def _rs(case):
    return np.random.RandomState((zlib.crc32(case_id(case).encode()) + SEED_SALT.get(case_id(case), 0)) & 0x7fffffff)


def inputs(case, cus=CUS):
    """the case's fp32 tensors (channels-last): hi / lo as the route needs them, w [clo][1][k][k] (x 0.2, as CONV_CASES), b_lo, b_hi,
    y_<side> / m_<side> of a folded operand, m_out of an output keep-mask.  A plain hi is a forward image: non-negative."""
    g, n, rs = case.geom, batch(case, cus), _rs(case)
    fside = case.fold[0] if case.fold is not None else None
    t = dict(n=n, w=(rs.standard_normal((g.clo, 1, g.k, g.k)) * 0.2).astype(f32), b_lo=rs.standard_normal(g.clo).astype(f32),
             b_hi=rs.standard_normal(1).astype(f32))
    if case.route in ('down', 'wgrad'):
        shape = (n, g.hh, g.hw, 1)
        t['hi'] = rs.standard_normal(shape).astype(f32) if fside == 'hi' else rs.random_sample(shape).astype(f32)
    if case.route in ('up', 'wgrad'):
        t['lo'] = rs.standard_normal((n, g.lh, g.lw, g.clo)).astype(f32)
    if fside is not None:
        _side, act, masked = case.fold
        shape = t[fside].shape
        y = rs.standard_normal(shape).astype(f32)
        m = (rs.random_sample(shape) >= 0.5).astype(np.uint8) if masked else None
        if act == 1:
            y = np.maximum(y, 0)                                 # a saved ReLU output
        if m is not None:
            y = y * m * 2.0                                      # ... of a layer with dropout: kept values times two
            t[f'm_{fside}'] = m
        t[f'y_{fside}'] = y.astype(f32)
    if case.out_mask:
        t['m_out'] = (rs.random_sample((n, g.lh, g.lw, g.clo) if case.route == 'down' else (n, g.hh, g.hw, 1)) >= 0.5).astype(np.uint8)
    return t


def operand(case, t, side, dtype, masked=True):
    """the hi / lo operand as multiplied, a torch tensor of `dtype` (masked=False: the keep-mask of a folded operand ignored)"""
    if case.fold is not None and case.fold[0] == side:
        return fold(t[side], t[f'y_{side}'], t.get(f'm_{side}') if masked else None, case.fold[1], dtype)
    return torch.from_numpy(t[side]).to(dtype)


def wants(case):
    return {'down': ('down',), 'up': ('up',), 'wgrad': ('dw', 'db1', 'db2')}[case.route]


# ---------------------------------------------------------------------------------------------------------------- reference (a): torch
def _nchw(a):
    return a.permute(0, 3, 1, 2)


def maps_torch(case, t, dtype, hi=None, lo=None):
    """the case's maps in torch on the CPU; hi / lo: operands as multiplied when they are not the case's own"""
    g = case.geom
    w = torch.from_numpy(t['w']).to(dtype)
    out = {}
    if case.route == 'down':
        hi = operand(case, t, 'hi', dtype) if hi is None else hi
        r = F.conv2d(_nchw(hi), w, torch.from_numpy(t['b_lo']).to(dtype) if case.bias else None, stride=g.s, padding=g.p).permute(0, 2, 3, 1)
        if case.out_mask:
            r = r * (2.0 * torch.from_numpy(t['m_out']).to(dtype))
        out['down'] = r.contiguous().numpy()
    elif case.route == 'up':
        lo = operand(case, t, 'lo', dtype) if lo is None else lo
        r = F.conv_transpose2d(_nchw(lo), w, torch.from_numpy(t['b_hi']).to(dtype) if case.bias else None, stride=g.s,
                               padding=g.p).permute(0, 2, 3, 1)
        if case.out_mask:
            r = r * (2.0 * torch.from_numpy(t['m_out']).to(dtype))
        out['up'] = r.contiguous().numpy()
    else:
        hi = operand(case, t, 'hi', dtype) if hi is None else hi
        lo = operand(case, t, 'lo', dtype) if lo is None else lo
        w.requires_grad_(True)
        F.conv2d(_nchw(hi), w, None, stride=g.s, padding=g.p).backward(_nchw(lo))          # dW of the Conv2d for the upstream gradient lo
        out.update(dw=w.grad.numpy(), db1=lo.sum((0, 1, 2)).numpy(), db2=hi.sum().numpy().reshape(()))
    return out


# ---------------------------------------------------------------------------------------------------------------- reference (b): numpy
def patches(hi, g):
    """[n * lh, lw, k * k] patch values of a single-channel map [n, hh, hw] (zero padded): the A operand of every product here"""
    hp = np.pad(hi, ((0, 0), (g.p, g.p), (g.p, g.p)))
    win = np.lib.stride_tricks.sliding_window_view(hp, (g.k, g.k), axis=(1, 2))[:, ::g.s, ::g.s][:, :g.lh, :g.lw]
    return np.ascontiguousarray(win).reshape(hi.shape[0] * g.lh, g.lw, g.k * g.k)


def col2im(tt, g, n):
    """hi [n, hh, hw] from T [n * lh, lw, k * k]: every output pixel gathers its taps"""
    hp = np.zeros((n, g.hh + 2 * g.p, g.hw + 2 * g.p), tt.dtype)
    tt = tt.reshape(n, g.lh, g.lw, g.k * g.k)
    for ky in range(g.k):
        for kx in range(g.k):
            hp[:, ky:ky + g.s * g.lh:g.s, kx:kx + g.s * g.lw:g.s] += tt[..., ky * g.k + kx]
    return hp[:, g.p:g.p + g.hh, g.p:g.p + g.hw]


def maps_numpy(case, t, hi=None, lo=None, w=None):
    """the same maps in numpy float64 by explicit patches: einsum over [row, position, tap]"""
    g, n = case.geom, t['n']
    w = (t['w'].astype(f64) if w is None else w).reshape(g.clo, g.k * g.k)
    out = {}
    if case.route in ('down', 'wgrad'):
        hi = operand(case, t, 'hi', torch.float64).numpy() if hi is None else hi
        pt = patches(hi[..., 0], g)
    if case.route in ('up', 'wgrad'):
        lo = (operand(case, t, 'lo', torch.float64).numpy() if lo is None else lo).reshape(n * g.lh, g.lw, g.clo)
    if case.route == 'down':
        r = np.einsum('rpt,ct->rpc', pt, w).reshape(n, g.lh, g.lw, g.clo)
        if case.bias:
            r = r + t['b_lo'].astype(f64)
        out['down'] = r * (2.0 * t['m_out']) if case.out_mask else r
    elif case.route == 'up':
        r = col2im(np.einsum('rpc,ct->rpt', lo, w), g, n)[..., None]
        if case.bias:
            r = r + t['b_hi'].astype(f64)
        out['up'] = r * (2.0 * t['m_out']) if case.out_mask else r
    else:
        out.update(dw=np.einsum('rpc,rpt->ct', lo, pt).reshape(g.clo, 1, g.k, g.k), db1=lo.sum((0, 1)), db2=f64(hi.sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------- 0-d condition
def scalar_margin(case, t):
    """|reference| of the case's 0-d output over sqrt(count) x rms of the summed values (>= 0.1 is asked), or None without a 0-d output"""
    if case.route != 'wgrad':
        return None
    hi = operand(case, t, 'hi', torch.float64).numpy()
    return abs(float(hi.sum())) / (np.sqrt(hi.size) * float(np.sqrt(np.mean(hi * hi))))


# ---------------------------------------------------------------------------------------------------------------- the streaming order
STREAM_WAVES, STREAM_GROUPS = 8, 256                           # WGS_WAVES / W1_WAVES; the cap of wgrad_c1_groups / wgrad_c1w_groups


def _chain(x, axis):
    """fp32 sum along an axis, one addition after the other"""
    return np.cumsum(x, axis=axis, dtype=f32).take(-1, axis=axis)


def _groups_sum(slabs):
    """slab_reduce_block (reduce.h): eight thread groups take the slabs z, z + 8, ... in order, then ((0+1)+(2+3)) + ((4+5)+(6+7))"""
    parts = [(_chain(slabs[z::8], 0) if z < len(slabs) else np.zeros(slabs.shape[1:], f32)) for z in range(8)]
    return ((parts[0] + parts[1]) + (parts[2] + parts[3])) + ((parts[4] + parts[5]) + (parts[6] + parts[7]))


def wgrad_stream(case, t):
    """wgrad_c1s_kernel / wgrad_c1w_kernel restated in fp32 numpy in their own order: a wave owns the lo rows wave + k n_waves and
    adds each row's positions four at a time (one MFMA) into one accumulator per (channel, tap); the workgroup's eight waves are
    added in order; the groups' slabs as slab_reduce_block adds them.  The bias sums the same way: a lane's chain over its rows and
    quads, the lanes of the workgroup in order, the groups."""
    g, n = case.geom, t['n']
    assert case.kernel in ('wgrad_c1s_kernel', C1W)
    lo = operand(case, t, 'lo', torch.float32).numpy().reshape(n * g.lh, g.lw, g.clo)
    hi = operand(case, t, 'hi', torch.float32).numpy()
    pt = patches(hi[..., 0], g)
    rows = n * g.lh
    groups = min((rows + STREAM_WAVES - 1) // STREAM_WAVES, STREAM_GROUPS)
    n_waves = groups * STREAM_WAVES
    slots = -(-g.lw // 4) * 4
    acc = np.zeros((n_waves, g.clo, g.k * g.k), f32)
    lo_sum = np.zeros((n_waves, 4, g.clo), f32)                   # a lane's chain: position slot (lane >> 4), channel
    # the image sum: each lo row brings the image rows that belong to it (s2: rows 2 r, 2 r + 1; s1: row r, and the last lo row of
    # an image its three extra rows); a lane's chain runs over its rows, then the workgroup's lanes in order
    own = g.s if g.s == 2 else 1
    img_rows = np.zeros((rows, own + g.k - 1, g.hw), f32)
    for r in range(g.lh):
        src = hi[:, g.s * r:g.s * r + own, :, 0]
        img_rows[r::g.lh, :own] = src
        if g.s == 1 and r == g.lh - 1:
            img_rows[r::g.lh, own:] = hi[:, r + 1:r + g.k, :, 0]
    img_sum = np.zeros((n_waves,) + img_rows.shape[1:], f32)
    for k in range(-(-rows // n_waves)):
        live = min(n_waves, rows - k * n_waves)
        rr = slice(k * n_waves, k * n_waves + live)
        for q in range(slots // 4):
            a, b = lo[rr, 4 * q:4 * q + 4], pt[rr, 4 * q:4 * q + 4]
            acc[:live] += np.einsum('wpc,wpt->wct', a, b, dtype=f32)
            lo_sum[:live, :a.shape[1]] += a
        img_sum[:live] += img_rows[rr]
    by_group = lambda x: x.reshape((groups, STREAM_WAVES) + x.shape[1:])
    dw = _groups_sum(_chain(by_group(acc), 1))
    db1 = _groups_sum(_chain(by_group(lo_sum).reshape(groups, STREAM_WAVES * 4, g.clo), 1))
    # (the image sum's lanes: the waves of a lane slot in order, then the butterfly over the lanes, numpy's pairwise sum here)
    db2 = _groups_sum(_chain(by_group(img_sum).reshape(groups, STREAM_WAVES, -1), 1).sum(1, dtype=f32)[:, None])[0]
    return dict(dw=dw.reshape(g.clo, 1, g.k, g.k), db1=db1, db2=np.asarray(db2, f32).reshape(()))


# ---------------------------------------------------------------------------------------------------------------- wrong kernels
def _f32(out):
    return {k: np.asarray(v, f64).astype(f32) for k, v in out.items()}


def _is(case, *kernels):
    return case.kernel in kernels


def _wrong_a(case, t):        # down c1: rows past the first grid pass (1024 workgroups x 4 waves) are missing
    out = maps_numpy(case, t)
    flat = out['down'].reshape(t['n'] * case.geom.lh, -1)
    flat[4096:] = 0.0
    return out


def _wrong_b(case, t):        # down c1: the neighbour of column 0 / 63 is the adjacent pixel instead of zero
    g = case.geom
    hi = operand(case, t, 'hi', torch.float64).numpy()[..., 0]
    hp = np.pad(np.pad(hi, ((0, 0), (0, 0), (1, 1)), mode='edge'), ((0, 0), (1, 1), (0, 0)))
    return maps_numpy(case._replace(geom=g._replace(p=0, hh=g.hh + 2, hw=g.hw + 2)), t, hi=hp[..., None])


def _wrong_c(case, t):        # down c1: image row -1 / 64 is read at the clamped index (element 0: the first image's row 0) instead of zero
    g = case.geom
    hi = operand(case, t, 'hi', torch.float64).numpy()[..., 0]
    hp = np.pad(hi, ((0, 0), (1, 1), (1, 1)))
    hp[:, 0, 1:-1] = hi[0, 0]
    hp[:, -1, 1:-1] = hi[0, 0]
    return maps_numpy(case._replace(geom=g._replace(p=0, hh=g.hh + 2, hw=g.hw + 2)), t, hi=hp[..., None])


def _wrong_d(case, t):        # up c1: the halo row between an image's two 16-row tiles is zero: hi rows 31 and 32 lose one lo row each
    out = maps_numpy(case, t)
    lo = operand(case, t, 'lo', torch.float64).numpy()
    plain = case._replace(bias=False, out_mask=False)
    for hy, ly in ((31, 16), (32, 15)):
        only = np.zeros_like(lo)
        only[:, ly] = lo[:, ly]
        out['up'][:, hy] -= maps_numpy(plain, t, lo=only)['up'][:, hy]
    return out


def _wrong_e(case, t, cus=CUS):        # up c1: tiles past the first pass (2 x CUs workgroups, 16 lo rows = 32 hi rows each) are missing
    out = maps_numpy(case, t)
    out['up'].reshape(-1, 32 * case.geom.hw)[2 * cus:] = 0.0
    return out


def _wrong_f(case, t):        # wgrad c1s: the second pass is missing (256 groups x 8 waves = 2048 rows)
    g, n = case.geom, t['n']
    hi, lo = operand(case, t, 'hi', torch.float64).numpy().copy(), operand(case, t, 'lo', torch.float64).numpy().copy()
    lo.reshape(n * g.lh, -1)[2048:] = 0.0
    out = maps_numpy(case, t, lo=lo)
    hi.reshape(n * g.lh, -1)[2048:] = 0.0                         # (a lo row brings its two image rows)
    out['db2'] = f64(hi.sum())
    return out


def _wrong_g(case, t):        # wgrad c1s: the image sum also counts the two halo rows 2 r - 1 and 2 r + 2 of every lo row
    out = maps_numpy(case, t)
    hi = operand(case, t, 'hi', torch.float64).numpy()
    out['db2'] = f64(2.0 * hi.sum() - hi[:, 0].sum() - hi[:, -1].sum())
    return out


def _wrong_h(case, t):        # wgrad c1w: the last lo row's three extra image rows are left out of the image sum
    out = maps_numpy(case, t)
    out['db2'] = f64(operand(case, t, 'hi', torch.float64).numpy()[:, :case.geom.lh].sum())
    return out


def _wrong_i(case, t):        # wgrad c1w: the seventh quad (positions 24 .. 27 of a lo row) is dropped
    lo = operand(case, t, 'lo', torch.float64).numpy().copy()
    lo[:, :, 24:] = 0.0
    return dict(maps_numpy(case, t, lo=lo), db2=maps_numpy(case, t)['db2'])


def _wrong_j(case, t):        # 1 -> 64 down: the positions of the last, partial 16-position tile are dropped
    g = case.geom
    out = maps_numpy(case, t)
    npos = g.lh * g.lw
    out['down'].reshape(t['n'], npos, g.clo)[:, npos // 16 * 16:] = 0.0
    return out


def _wrong_k(case, t):        # 1 -> 64 down, 3 x 3: taps 9 - 15 read on into the next channel's weights (and the image rows 3 .. 5 below)
    g = case.geom
    assert g.k == 3 and g.s == 1
    w = np.concatenate([t['w'].astype(f64).ravel(), np.zeros(16)])
    w16 = np.stack([w[9 * c:9 * c + 16] for c in range(g.clo)])
    hi = operand(case, t, 'hi', torch.float64).numpy()[..., 0]
    hp = np.pad(hi, ((0, 0), (g.p, g.p + 3), (g.p, g.p)))          # zero outside the image: the kernel's range check holds
    pt = np.stack([hp[:, tap // 3:tap // 3 + g.lh, tap % 3:tap % 3 + g.lw] for tap in range(16)], -1)
    r = np.einsum('nyxt,ct->nyxc', pt, w16) + (t['b_lo'].astype(f64) if case.bias else 0.0)
    return dict(down=r * (2.0 * t['m_out']) if case.out_mask else r)


def _wrong_l(case, t):        # up KQ = 2: only the first 16 channels are multiplied
    lo = operand(case, t, 'lo', torch.float64).numpy().copy()
    lo[..., 16:] = 0.0
    return maps_numpy(case, t, lo=lo)


def _wrong_m(case, t):        # folded operand: the keep-mask is ignored
    side = case.fold[0]
    return maps_numpy(case, t, **{side: operand(case, t, side, torch.float64, masked=False).numpy()})


C1S = 'wgrad_c1s_kernel'
# name -> (builder, the cases it applies to, the cases among them that reach its edge: it fails exactly those)
WRONG_KERNELS = {
    'a: down c1, rows past the first grid pass missing': (_wrong_a, lambda c: _is(c, 'down_c1s_kernel<0>'), lambda c: batch(c) * 32 > 4096),
    'b: down c1, adjacent pixel beside column 0 / 63': (_wrong_b, lambda c: _is(c, 'down_c1s_kernel<0>'), lambda c: True),
    'c: down c1, clamped index for image row -1 / 64': (_wrong_c, lambda c: _is(c, 'down_c1s_kernel<0>'), lambda c: True),
    'd: up c1, zero halo row between the two tiles': (_wrong_d, lambda c: _is(c, 'up_c1_kernel<0, false>'), lambda c: True),
    'e: up c1, tiles past the first pass missing': (_wrong_e, lambda c: _is(c, 'up_c1_kernel<0, false>'), lambda c: 2 * batch(c) > 2 * CUS),
    'f: wgrad c1s, second pass missing': (_wrong_f, lambda c: _is(c, C1S), lambda c: batch(c) * 32 > 2048),
    'g: wgrad c1s, halo rows in the image sum': (_wrong_g, lambda c: _is(c, C1S), lambda c: True),
    'h: wgrad c1w, last row\'s extra image rows not summed': (_wrong_h, lambda c: _is(c, C1W), lambda c: True),
    'i: wgrad c1w, seventh quad dropped': (_wrong_i, lambda c: _is(c, C1W), lambda c: c.geom.lw > 24),
    'j: 1 -> 64 down, last partial tile dropped': (_wrong_j, lambda c: _is(c, DOWN64), lambda c: c.geom.lh * c.geom.lw % 16 != 0),
    'k: 1 -> 64 down 3 x 3, taps 9 - 15 from the next channel': (_wrong_k, lambda c: _is(c, DOWN64) and c.geom.k == 3, lambda c: True),
    'l: up KQ = 2, first 16 channels only': (_wrong_l, lambda c: _is(c, UP2), lambda c: True),
    'm: folded operand, keep-mask ignored': (_wrong_m, lambda c: c.fold is not None and c.fold[2] and c.kernel != GENERIC, lambda c: True),
}


def wrong_kernel(name, case, t):
    return _f32(WRONG_KERNELS[name][0](case, t))

"""Case tables, float64 references, fp32 yardstick, CPU model and the bar of the float64 accuracy tests of the 32 <-> 32 channel
k4 s2 p1 links (ar-vae_amd/csrc/conv32.hip, down32p.h, wgrad32r.h): the hot path of the dSprites step.  Shared by the GPU test
(test_conv32_links_float64.py) and by the CPU test that proves the references right and the table sharp (test_conv32_cases.py).
No test in here.

The bar, for every output tensor:          e_got <= R * e_cpu + FLOOR                      (split_cases.py; relative L2 to float64)
for the forward routes also PER IMAGE:     e_got[i] <= R_IMAGE * e_cpu[i] + FLOOR          (image i's own distances and norm)
R = 4 and FLOOR = 1e-7 are split_cases.py's; R_IMAGE = R: nothing had to be derived.  Measured on the CPU (torch 16 threads; model =
the kernels' scaled two-term fp16 product with float64 accumulation, model(); ratios e / e_cpu and the share of the bar used):

  reduction length             model e / e_cpu (share of bar)           least harmful defect (e: one product l h' missing)
  down  512                    0.20 - 0.25  (<= 0.06; image <= 0.09)    1.8e-4 - 2.1e-4, 120 - 142 x its bar (an image: 123 - 197 x)
  up    128                    0.44 - 0.94  (<= 0.20; image <= 0.14)    1.3e-4 - 2.2e-4, 228 - 331 x (an image: 230 - 372 x)
  wgrad n lo lo = 16 .. 16400  0.07 - 1.28  (<= 0.22)                   5.4e-5 - 2.2e-4, 43 x (9472 pixels) - 555 x
(torch's own fp32 error: 3.1e-7 - 4.0e-7 down, 0.9e-7 - 1.6e-7 up; for dW it grows from 7e-8 at 16 pixels to 1.2e-6 at 9472 and
1.0e-6 at 16400, where the model stays at 5.5e-8 - 8.6e-8.  Every other defect of WRONG_KERNELS is at least 2e-2 off.)

Pixel counts of the weight gradient.  The three-term bf16 kernels of split_cases.py lose the separation after a few thousand terms
because the product they can lose is 2^-16 of the result.  In the two-term fp16 product l is 11 bits below h: a missing l h' is
about 2e-4 off at every length, while torch's fp32 accumulation is 1.2e-6 off at 1e4 pixels and grows like sqrt(K): four times that
meets 2e-4 near K = 2e7 pixels.  Every pixel count of this table (at most 16400 = 1025 x 4 x 4) is far inside, so the n = 1024 and
n = 1025 cases carry the arithmetic defects as well as the structural ones (their `why` says so).

A case is a Case tuple:
  route      'down'  lo = act(conv(hi) + b)             -> {'down'}
             'up'    hi = act(conv_transpose(lo) + b)   -> {'up'}
             'wgrad' dW of the Conv2d for the upstream gradient lo, and the bias sums -> {'dw', 'db' (bias_side 1: sums of lo, 2: of hi)}
  lo         16 / 8 / 4 (hi = 2 lo); 2 only outside the kernels
  n          an int or an expression in `cus`, resolved by batch(case, cus): cus = 256 on the MI355X; the GPU test passes
             multi_processor_count capped as grid_for_tiles caps it (min(cus, AMAX_N / 4))
  bias, act  forward routes: bias or none; 'none' / 'relu' ('selu' only outside).  ReLU is applied to each result's own
             pre-activation: the map is 1-Lipschitz, nothing is masked or left out
  bias_side  wgrad: 0 / 1 / 2
  accumulate wgrad: dw and db hold non-zero values before the call; the expected result is prior + gradient
  amax_tail  None / 'hi' / 'lo': that operand's largest magnitude is 64 x the rest and sits in the tensor's last 16 bytes
  kernel     the kernel the case is meant to reach (test_conv32_cases.py holds it to launch(), the host code restated)
  outside    None, or what puts the case one step outside conv32_fits / the per-layer predicates: 'out_mask', 'fold_hi', 'fold_lo'

  launch(route, lo, n, cus)    tiles_for / grid_for_tiles / down_small_grid / launch_up_v / conv32_wgrad_groups restated
  inputs(case, cus)            fp32 tensors, channels-last, seeded by the case's id
  maps_torch(case, t, dtype)   reference (a): torch on the CPU, float64 the reference, float32 the yardstick
  maps_numpy(case, t)          reference (b): numpy float64 by explicit patches (im2col, einsum, col2im)
  model(case, t)               the kernels' arithmetic on the case's own im2col matrices: test_two_term_arithmetic.matmul_two_term
  hold(...)                    both forms of the bar, every figure printed
  WRONG_KERNELS                deliberate defects built from reference (b) or from the model"""
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import test_two_term_arithmetic as tt
from loss_cases import rel
from single_channel_cases import SELU_SA, SELU_SCALE, fold
from split_cases import FLOOR, R

f32, f64 = np.float32, np.float64
CUS = 256                                                     # compute units of the MI355X
AMAX_N = 1024                                                 # amax.h
R_IMAGE = R                                                   # the per-image form needs no value of its own (docstring)
C = 32                                                        # channels on both sides

Case = namedtuple('Case', 'route lo n bias act bias_side accumulate amax_tail kernel why outside')


# ---------------------------------------------------------------------------------------------------------------- the host code
Launch = namedtuple('Launch', 'kernel px ti tiles grid per_wg')


def tile_images(lo, px):
    """Tile<LO, PX> (conv32_common.h): (images per tile TI, rows of one image per tile TR)"""
    rows = px // lo
    return (rows // lo, lo) if rows > lo else (1, rows)


def tiles_for(lo, px, n):
    ti, tr = tile_images(lo, px)
    return n * (lo // tr) if ti == 1 else -(-n // ti)


def grid_for_tiles(tiles, cus):
    return min(tiles, min(cus, AMAX_N // 4))


def down_small_grid(tiles, cus):
    return min(tiles, 2 * cus, AMAX_N)


def launch(route, lo, n, cus=CUS):
    """what conv32_down / conv32_up (launch_up_v) / conv32_wgrad launch for a batch: kernel, lo pixels per tile, images per tile,
    tiles, workgroups, and the tiles of a workgroup's contiguous run (per_wg > 1: the persistent loop runs again)"""
    if route == 'down':
        px = 32 if lo == 4 else 64
        tiles = tiles_for(lo, px, n)
        grid = down_small_grid(tiles, cus) if lo == 4 else grid_for_tiles(tiles, cus)
        kernel = 'down32s_kernel<4>' if lo == 4 else f'down32p_kernel<{lo}>'
    elif route == 'up':
        small = (lo == 4 and 2 * tiles_for(4, 128, n) <= cus) or (lo == 8 and tiles_for(8, 128, n) <= cus)
        px = 32 if small else 128
        tiles = tiles_for(lo, px, n)
        grid = grid_for_tiles(tiles, cus)
        kernel = 'up32p_kernel' if lo == 16 else f'up32x_kernel<{lo},.,{px}>'
    elif lo == 4:
        px, tiles = 64, tiles_for(4, 64, n)
        grid = grid_for_tiles(tiles, cus)
        kernel = 'wgrad32x_kernel<4>'
    else:                                                         # stream_geometry: steps of 32 lo pixels
        px, tiles = 32, n * (lo * lo // 32)
        spw = max(-(-tiles // cus), 1)
        return Launch(f'wgrad32r_kernel<{lo}>', px, 1, tiles, -(-tiles // spw), spw)
    return Launch(kernel, px, tile_images(lo, px)[0], tiles, grid, -(-tiles // grid))


# ---------------------------------------------------------------------------------------------------------------- cases
def _c(route, lo, n, kernel, why, bias=True, act='relu', bias_side=1, accumulate=False, amax_tail=None, outside=None):
    if route == 'wgrad':
        bias, act = False, 'none'
    else:
        bias_side, accumulate = 0, False
    return Case(route, lo, n, bias, act, bias_side, accumulate, amax_tail, kernel, why, outside)


D16, D8, D4 = 'down32p_kernel<16>', 'down32p_kernel<8>', 'down32s_kernel<4>'
U16, U8S, U8L, U4S, U4L = 'up32p_kernel', 'up32x_kernel<8,.,32>', 'up32x_kernel<8,.,128>', 'up32x_kernel<4,.,32>', 'up32x_kernel<4,.,128>'
W16, W8, W4 = 'wgrad32r_kernel<16>', 'wgrad32r_kernel<8>', 'wgrad32x_kernel<4>'

DOWN_CASES = [
    _c('down', 16, 1, D16, 'four tiles on four workgroups', bias=False, act='none'),
    _c('down', 16, 3, D16, 'twelve tiles'),
    _c('down', 16, 'cus//4', D16, 'the last single pass: a tile per workgroup'),
    _c('down', 16, 'cus//4+1', D16, 'the first second pass: runs of two tiles, half the workgroups idle', act='none'),
    _c('down', 16, 'cus//2+2', D16, 'runs of three tiles: they start inside an image, the last run is short'),
    _c('down', 16, 'cus//2+2', D16, 'the same with the maximum in the last 16 bytes: the AMAX pass of a tensor of more than 1024 blocks',
       amax_tail='hi'),
    _c('down', 8, 1, D8, 'one tile', act='none'),
    _c('down', 8, 3, D8, 'three tiles', bias=False),
    _c('down', 8, 'cus', D8, 'the last single pass'),
    _c('down', 8, 'cus+1', D8, 'the first second pass: runs of two images'),
    _c('down', 4, 1, D4, 'half a tile: the second image is past the batch', act='none'),
    _c('down', 4, 3, D4, 'two tiles, the last partial'),
    _c('down', 4, '4*cus', D4, 'the last single pass on 2 cus workgroups', bias=False),
    _c('down', 4, '4*cus+1', D4, 'the first second pass; the last tile partial'),
]
UP_CASES = [
    _c('up', 16, 1, U16, 'two tiles', bias=False, act='none'),
    _c('up', 16, 3, U16, 'six tiles'),
    _c('up', 16, 'cus//2', U16, 'the last single pass'),
    _c('up', 16, 'cus//2+1', U16, 'the first second pass: both LDS images', act='none'),
    _c('up', 8, 1, U8S, 'two half-image tiles', act='none'),
    _c('up', 8, 3, U8S, 'six tiles', bias=False),
    _c('up', 8, 'cus//2', U8S, 'the last single pass of the 32-pixel tiles'),
    _c('up', 8, 'cus//2+1', U8S, 'their first second pass'),
    _c('up', 8, '2*cus', U8S, 'the last batch on 32-pixel tiles: runs of four', act='none'),
    _c('up', 8, '2*cus+1', U8L, 'the first batch on 128-pixel tiles (two images): odd, the last tile partial, runs of two'),
    _c('up', 8, '2*cus+1', U8L, 'the same with the maximum in the last 16 bytes', amax_tail='lo', act='none'),
    _c('up', 8, '2*cus+2', U8L, '128-pixel tiles, even: no partial tile'),
    _c('up', 4, 1, U4S, 'half a tile', act='none'),
    _c('up', 4, 3, U4S, 'two tiles, the last partial', bias=False),
    _c('up', 4, '2*cus', U4S, 'the last single pass of the 32-pixel tiles'),
    _c('up', 4, '2*cus+1', U4S, 'their first second pass, the last tile partial'),
    _c('up', 4, '4*cus', U4S, 'the last batch on 32-pixel tiles', act='none'),
    _c('up', 4, '4*cus+1', U4L, 'the first batch on 128-pixel tiles (eight images): one image in the last tile'),
    _c('up', 4, '8*cus', U4L, 'the last single pass of the 128-pixel tiles, all full', bias=False),
    _c('up', 4, '8*cus+1', U4L, 'their first second pass; one image in the last tile'),
]
WGRAD_CASES = [
    _c('wgrad', 4, 1, W4, 'a quarter of a tile'),
    _c('wgrad', 4, 2, W4, 'half a tile', bias_side=2),
    _c('wgrad', 4, 3, W4, 'three images of four', bias_side=0),
    _c('wgrad', 4, 3, W4, 'three images of four', bias_side=1, accumulate=True),
    _c('wgrad', 4, 3, W4, 'three images of four', bias_side=2),
    _c('wgrad', 4, 4, W4, 'exactly one tile'),
    _c('wgrad', 4, 5, W4, 'two tiles, one image in the last', bias_side=0, accumulate=True),
    _c('wgrad', 4, 5, W4, 'two tiles, one image in the last', bias_side=1),
    _c('wgrad', 4, 5, W4, 'two tiles, one image in the last', bias_side=2, accumulate=True),
    _c('wgrad', 4, 5, W4, 'the maximum of lo in its last 16 bytes', bias_side=1, amax_tail='lo'),
    _c('wgrad', 4, 5, W4, 'the maximum of hi in its last 16 bytes', bias_side=2, amax_tail='hi'),
    _c('wgrad', 4, '4*cus', W4, 'the last single pass: 16384 pixels, inside the separation (docstring): all defects'),
    _c('wgrad', 4, '4*cus+1', W4, 'the first second pass, one image in the last tile: 16400 pixels, inside the separation: all defects',
       bias_side=2),
    _c('wgrad', 16, 3, W16, 'the row stream without a bias sum', bias_side=0),
    _c('wgrad', 16, 37, W16, 'the row stream without a bias sum: steps that start inside an image', bias_side=0),
    _c('wgrad', 16, 3, W16, 'the row stream into a non-zero dw / db', bias_side=1, accumulate=True),
    _c('wgrad', 8, 3, W8, 'the row stream without a bias sum', bias_side=0),
    _c('wgrad', 8, 37, W8, 'the row stream without a bias sum: 74 steps', bias_side=0),
    _c('wgrad', 8, 3, W8, 'the row stream into a non-zero dw / db', bias_side=2, accumulate=True),
]
# ---- one step outside conv32_fits or the per-layer predicates of link_gemm.hip: the generic kernel, held to the same bar
GENERIC = 'link_gemm_kernel'
OUTSIDE_CASES = [
    _c('down', 8, 3, GENERIC, 'an output keep-mask', act='none', outside='out_mask'),
    _c('up', 8, 3, GENERIC, 'an output keep-mask', act='none', outside='out_mask'),
    _c('down', 8, 3, GENERIC, 'hi = (g, y, ReLU)', outside='fold_hi'),
    _c('up', 8, 3, GENERIC, 'lo = (g, y, ReLU)', outside='fold_lo'),
    _c('wgrad', 8, 3, GENERIC, 'lo = (g, y, ReLU)', outside='fold_lo'),
    _c('wgrad', 4, 3, GENERIC, 'hi = (g, y, ReLU)', bias_side=2, outside='fold_hi'),
    _c('down', 4, 3, GENERIC, 'SELU', act='selu'),
    _c('up', 4, 3, GENERIC, 'SELU', act='selu'),
    _c('down', 2, 3, GENERIC, 'lo size 2'),
    _c('up', 2, 3, GENERIC, 'lo size 2'),
    _c('wgrad', 2, 3, GENERIC, 'lo size 2'),
]
CASES = DOWN_CASES + UP_CASES + WGRAD_CASES + OUTSIDE_CASES


def batch(case, cus=CUS):
    return int(case.n) if isinstance(case.n, int) else int(eval(case.n, {'__builtins__': {}}, {'cus': cus}))


def case_id(case):
    """route and lo size, the batch at cus = 256 (and its expression), the kernel, then what differs from the plain case"""
    tag = f'{case.route}{case.lo}-n{batch(case)}'
    if not isinstance(case.n, int):
        tag += f'({case.n.replace("//", "/").replace("*", "")})'
    tag += f'-{case.kernel}'
    if case.route == 'wgrad':
        tag += f'-side{case.bias_side}' + ('-accumulate' if case.accumulate else '')
    else:
        tag += f'-{case.act}' + ('' if case.bias else '-nobias')
    if case.amax_tail:
        tag += f'-tail_{case.amax_tail}'
    if case.outside:
        tag += f'-{case.outside}'
    return tag


assert len({case_id(c) for c in CASES}) == len(CASES)


def _rs(case):
    return np.random.RandomState(zlib.crc32(case_id(case).encode()) & 0x7fffffff)


def inputs(case, cus=CUS):
    """the case's fp32 tensors (channels-last): hi / lo as the route needs them, w [clo][chi][4][4] (x 0.1), b, y_<side> of a folded
    operand, m_out of an output keep-mask, dw0 / db0 of an accumulating weight gradient (of the gradient's own size)"""
    n, lo, rs = batch(case, cus), case.lo, _rs(case)
    t = dict(n=n, w=(rs.standard_normal((C, C, 4, 4)) * 0.1).astype(f32), b=rs.standard_normal(C).astype(f32))
    if case.route in ('down', 'wgrad'):
        t['hi'] = rs.standard_normal((n, 2 * lo, 2 * lo, C)).astype(f32)
    if case.route in ('up', 'wgrad'):
        t['lo'] = rs.standard_normal((n, lo, lo, C)).astype(f32)
    if case.amax_tail:
        x = t[case.amax_tail].reshape(-1)
        x[-2] = 0.0
        x[-2] = -64.0 * np.abs(x).max()
    if case.outside in ('fold_hi', 'fold_lo'):
        side = case.outside[-2:]
        t[f'y_{side}'] = np.maximum(rs.standard_normal(t[side].shape), 0).astype(f32)        # a saved ReLU output
    if case.outside == 'out_mask':
        t['m_out'] = (rs.random_sample((n, lo, lo, C) if case.route == 'down' else (n, 2 * lo, 2 * lo, C)) >= 0.5).astype(np.uint8)
    if case.accumulate:
        scale = np.sqrt(n * lo * lo)
        t['dw0'] = (rs.standard_normal((C, C, 4, 4)) * scale).astype(f32)
        t['db0'] = (rs.standard_normal(C) * scale * case.bias_side).astype(f32)
    return t


def operand(case, t, side, dtype):
    """the hi / lo operand as multiplied, a torch tensor of `dtype`"""
    if case.outside == f'fold_{side}':
        return fold(t[side], t[f'y_{side}'], None, 1, dtype)
    return torch.from_numpy(t[side]).to(dtype)


def wants(case):
    return (case.route,) if case.route != 'wgrad' else ('dw', 'db') if case.bias_side else ('dw',)


# ---------------------------------------------------------------------------------------------------------------- reference (a): torch
def _nchw(a):
    return a.permute(0, 3, 1, 2)


def _act_torch(r, act):
    if act == 'relu':
        return F.relu(r)
    if act == 'selu':                                             # the kernels' fp32 constants (common.h): the SAME operation
        return torch.where(r > 0, SELU_SCALE * r, SELU_SA * torch.expm1(r))
    return r


def maps_torch(case, t, dtype):
    w = torch.from_numpy(t['w']).to(dtype)
    b = torch.from_numpy(t['b']).to(dtype) if case.bias else None
    if case.route == 'wgrad':
        hi, lo = operand(case, t, 'hi', dtype), operand(case, t, 'lo', dtype)
        w.requires_grad_(True)
        F.conv2d(_nchw(hi), w, None, stride=2, padding=1).backward(_nchw(lo))             # dW of the Conv2d for the upstream gradient lo
        out = dict(dw=w.grad)
        if case.bias_side:
            out['db'] = (lo if case.bias_side == 1 else hi).sum((0, 1, 2))
        if case.accumulate:
            out = {k: torch.from_numpy(t[k + '0']).to(dtype) + v for k, v in out.items()}
        return {k: v.numpy() for k, v in out.items()}
    if case.route == 'down':
        r = F.conv2d(_nchw(operand(case, t, 'hi', dtype)), w, b, stride=2, padding=1)
    else:
        r = F.conv_transpose2d(_nchw(operand(case, t, 'lo', dtype)), w, b, stride=2, padding=1)
    r = _act_torch(r, case.act).permute(0, 2, 3, 1)
    if case.outside == 'out_mask':
        r = r * (2.0 * torch.from_numpy(t['m_out']).to(dtype))
    return {case.route: r.contiguous().numpy()}


# ---------------------------------------------------------------------------------------------------------------- reference (b): numpy
TAPS = [(ky, kx) for ky in range(4) for kx in range(4)]


def im2col(hi, mode='constant'):
    """[n lo lo, 16 taps x 32 channels] patches of hi [n, 2 lo, 2 lo, 32], zero padded (mode='edge': the adjacent pixel instead)"""
    n, hh = hi.shape[0], hi.shape[1]
    hp = np.pad(hi, ((0, 0), (1, 1), (1, 1), (0, 0)), mode=mode)
    return np.stack([hp[:, ky:ky + hh:2, kx:kx + hh:2] for ky, kx in TAPS], 3).reshape(n * (hh // 2) ** 2, 16 * C)


def col2im(tt_, n, lo):
    """hi [n, 2 lo, 2 lo, 32] from T [n lo lo, 16, 32]: every lo pixel scatters its taps"""
    hp = np.zeros((n, 2 * lo + 2, 2 * lo + 2, C), tt_.dtype)
    tt_ = tt_.reshape(n, lo, lo, 16, C)
    for i, (ky, kx) in enumerate(TAPS):
        hp[:, ky:ky + 2 * lo:2, kx:kx + 2 * lo:2] += tt_[:, :, :, i]
    return hp[:, 1:-1, 1:-1]


def up_cols(lo_t, w, mode='constant'):
    """the up map as four products, one per stride-parity class (py, px): -> [((py, px), A [n lo lo, 4 x 32], B [4 x 32, 32])].
    hi pixel (2 y + py, 2 x + px) gathers the lo pixels (y + dy, x + dx) of the taps with ky = py + 1 - 2 dy, kx = px + 1 - 2 dx"""
    n, lo = lo_t.shape[0], lo_t.shape[1]
    lp = np.pad(lo_t, ((0, 0), (1, 1), (1, 1), (0, 0)), mode=mode)
    out = []
    for py in (0, 1):
        for px in (0, 1):
            a, b = [], []
            for ky in range((py + 1) % 2, 4, 2):
                for kx in range((px + 1) % 2, 4, 2):
                    dy, dx = (py + 1 - ky) // 2, (px + 1 - kx) // 2
                    a.append(lp[:, 1 + dy:1 + dy + lo, 1 + dx:1 + dx + lo].reshape(n * lo * lo, C))
                    b.append(w[:, :, ky, kx])                     # [clo, chi]
            out.append(((py, px), np.concatenate(a, 1), np.concatenate(b, 0)))
    return out


def _act_numpy(r, act):
    if act == 'relu':
        return np.maximum(r, 0)
    if act == 'selu':
        return np.where(r > 0, SELU_SCALE * r, SELU_SA * np.expm1(np.minimum(r, 0)))
    return r


def _epilogue(case, t, r):
    """bias, activation, keep-mask on a forward pre-activation, in r's own dtype"""
    if case.bias:
        r = r + t['b'].astype(r.dtype)
    r = _act_numpy(r, case.act)
    return r * (2 * t['m_out']).astype(r.dtype) if case.outside == 'out_mask' else r


def _finish_wgrad(case, t, dw, lo, hi):
    out = dict(dw=dw.reshape(C, C, 4, 4))
    if case.bias_side:
        out['db'] = (lo if case.bias_side == 1 else hi).reshape(-1, C).sum(0)
    if case.accumulate:
        out = {k: t[k + '0'].astype(f64) + v for k, v in out.items()}
    return out


def maps_numpy(case, t, hi=None, lo=None, mode='constant'):
    """the same maps in numpy float64 by explicit patches; hi / lo: operands as multiplied when they are not the case's own"""
    n, lo_size = t['n'], case.lo
    w = t['w'].astype(f64)
    wm = w.transpose(2, 3, 1, 0).reshape(16 * C, C)                # [(tap, chi), clo]
    if case.route in ('down', 'wgrad'):
        hi = operand(case, t, 'hi', torch.float64).numpy() if hi is None else hi
    if case.route in ('up', 'wgrad'):
        lo = operand(case, t, 'lo', torch.float64).numpy() if lo is None else lo
    if case.route == 'down':
        r = np.einsum('pk,ko->po', im2col(hi, mode), wm, optimize=True).reshape(n, lo_size, lo_size, C)
        return dict(down=_epilogue(case, t, r))
    if case.route == 'up':
        if mode == 'constant':
            r = col2im(np.einsum('po,oct->ptc', lo.reshape(-1, C), w.reshape(C, C, 16), optimize=True), n, lo_size)
        else:                                                     # (the gather form: a border tap has a pixel to read)
            r = np.zeros((n, 2 * lo_size, 2 * lo_size, C))
            for (py, px), a, b in up_cols(lo, w, mode):
                r[:, py::2, px::2] = np.einsum('pk,kc->pc', a, b, optimize=True).reshape(n, lo_size, lo_size, C)
        return dict(up=_epilogue(case, t, r))
    dw = np.einsum('po,pk->ok', lo.reshape(-1, C), im2col(hi, mode), optimize=True)       # [clo, (tap, chi)]
    return _finish_wgrad(case, t, dw.reshape(C, 16, C).transpose(0, 2, 1), lo, hi)


# ---------------------------------------------------------------------------------------------------------------- the model
def _two_term(a, b, amax_a, amax_b, drop_lh=False):
    """test_two_term_arithmetic.matmul_two_term with the operands' maxima given (the scale is the whole TENSOR's) and, for the
    defect, without the product l h'.  test_conv32_cases.py holds it to matmul_two_term bit for bit"""
    (sa, ia), (sb, ib) = tt.pow2_for(amax_a), tt.pow2_for(amax_b)
    with np.errstate(over='ignore', invalid='ignore'):
        ya, yb = (a * sa).astype(f32), (b * sb).astype(f32)
        ah, bh = ya.astype(np.float16), yb.astype(np.float16)
        al, bl = (ya - ah.astype(f32)).astype(np.float16), (yb - bh.astype(f32)).astype(np.float16)
        acc = ah.astype(f64) @ bl.astype(f64) + ah.astype(f64) @ bh.astype(f64)
        if not drop_lh:
            acc = al.astype(f64) @ bh.astype(f64) + acc
        return (acc * f64(ia) * f64(ib)).astype(f32)


def _pinned(a, b, amax_b):
    """a zero column against a row that holds max |w|: the product is unchanged and matmul_two_term scales b as the whole tensor"""
    a = np.concatenate([a, np.zeros((a.shape[0], 1), f32)], 1)
    row = np.zeros((1, b.shape[1]), f32)
    row[0, 0] = amax_b
    return a, np.concatenate([b, row], 0)


def model(case, t, drop_lh=False, tail_missed=False):
    """the scaled two-term fp16 product (splitmath.h) on the case's own im2col matrices, fp32 epilogue: the 'correct kernel' of the
    CPU test.  drop_lh / tail_missed: the two arithmetic defects (the second takes an operand's scale without its last 16 bytes)"""
    assert case.kernel != GENERIC
    n, lo_size = t['n'], case.lo
    amax = lambda x: f32(np.abs(x.reshape(-1)[:-4] if tail_missed else x).max())
    plain = not (drop_lh or tail_missed)
    if case.route == 'down':
        a, b = im2col(t['hi']), np.ascontiguousarray(t['w'].transpose(2, 3, 1, 0).reshape(16 * C, C))
        r = tt.matmul_two_term(a, b) if plain else _two_term(a, b, amax(t['hi']), np.abs(b).max(), drop_lh)
        return dict(down=_epilogue(case, t, r.reshape(n, lo_size, lo_size, C)))
    if case.route == 'up':
        r = np.zeros((n, 2 * lo_size, 2 * lo_size, C), f32)
        wmax = np.abs(t['w']).max()
        for (py, px), a, b in up_cols(t['lo'], t['w']):
            p = tt.matmul_two_term(*_pinned(a, b, wmax)) if plain else _two_term(a, b, amax(t['lo']), wmax, drop_lh)
            r[:, py::2, px::2] = p.reshape(n, lo_size, lo_size, C)
        return dict(up=_epilogue(case, t, r))
    a, b = np.ascontiguousarray(t['lo'].reshape(-1, C).T), im2col(t['hi'])
    dw = tt.matmul_two_term(a, b) if plain else _two_term(a, b, amax(t['lo']), amax(t['hi']), drop_lh)
    out = dict(dw=np.ascontiguousarray(dw.reshape(C, 16, C).transpose(0, 2, 1)).reshape(C, C, 4, 4))
    if case.bias_side:
        out['db'] = t['lo' if case.bias_side == 1 else 'hi'].astype(f64).reshape(-1, C).sum(0).astype(f32)
    if case.accumulate:
        out = {k: t[k + '0'] + v for k, v in out.items()}
    return out


# ---------------------------------------------------------------------------------------------------------------- the bar
def rel_images(x, ref):
    """relative L2 distance per image (axis 0); an all-zero reference image is met only by an all-zero result"""
    x, ref = np.asarray(x, f64).reshape(len(ref), -1), np.asarray(ref, f64).reshape(len(ref), -1)
    d, nrm = np.linalg.norm(x - ref, axis=1), np.linalg.norm(ref, axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(d == 0, 0.0, np.where(nrm == 0, np.inf, d / nrm))


def hold(cid, got, cpu, ref, say=print):
    """both forms of the bar on every output of the reference; -> list of what misses it.  Prints each figure first."""
    bad = []
    for k, want in ref.items():
        g = np.asarray(got[k])
        if not np.all(np.isfinite(g)):
            say(f'{cid} {k}: not finite')
            bad.append((k, 'not finite'))
            continue
        e_got, e_cpu = rel(g, want), rel(cpu[k], want)
        ratio = e_got / e_cpu if e_cpu > 0 else float('inf' if e_got > 0 else 0)
        say(f'{cid} {k}: e_hip {e_got:.3e}  e_cpu {e_cpu:.3e}  e_hip/e_cpu {ratio:.2f}  bar {R * e_cpu + FLOOR:.3e}')
        if not e_got <= R * e_cpu + FLOOR:
            bad.append((k, e_got, e_cpu))
        if k in ('down', 'up'):
            ei_got, ei_cpu = rel_images(g, want), rel_images(cpu[k], want)
            share = ei_got / (R_IMAGE * ei_cpu + FLOOR)
            i = int(np.argmax(share))
            say(f'{cid} {k} per image: worst image {i}  e_hip {ei_got[i]:.3e}  e_cpu {ei_cpu[i]:.3e}  bar {R_IMAGE * ei_cpu[i] + FLOOR:.3e}  '
                f'share {share[i]:.2f}')
            if not np.all(ei_got <= R_IMAGE * ei_cpu + FLOOR):
                miss = np.flatnonzero(~(ei_got <= R_IMAGE * ei_cpu + FLOOR))
                bad.append((k, 'images', miss[:8].tolist(), len(miss), float(ei_got[i]), float(ei_cpu[i])))
    return bad


# ---------------------------------------------------------------------------------------------------------------- wrong kernels
def _f32(out):
    return {k: np.asarray(v, f64).astype(f32) for k, v in out.items()}


def _conv32(case):
    return case.kernel != GENERIC


def _forward(case):
    return _conv32(case) and case.route != 'wgrad'


def _wrong_first_tile_only(case, t):      # a workgroup multiplies the first tile of its run and leaves: tiles past the first pass missing
    la = launch(case.route, case.lo, t['n'])
    if case.route == 'wgrad':             # (wgrad32x_kernel<4>: a tile is four images; what it misses is not summed)
        dead = (np.arange(t['n']) // la.ti) % la.per_wg != 0
        lo, hi = t['lo'].astype(f64), t['hi'].astype(f64)
        lo[dead], hi[dead] = 0.0, 0.0
        return maps_numpy(case, t, hi=hi, lo=lo)
    out = maps_numpy(case, t)[case.route]
    rows = out.reshape(-1, C)                                     # output pixels: la.px of them per tile going down, 4 la.px going up
    per_tile = la.px if case.route == 'down' else 4 * la.px
    rows[(np.arange(len(rows)) // per_tile) % la.per_wg != 0] = 0.0
    return {case.route: out}


def _wrong_partial_tile_dropped(case, t):  # tiles = n / TI rounded DOWN: the images of a last partial tile are never multiplied
    la = launch(case.route, case.lo, t['n'])
    full = t['n'] // la.ti * la.ti
    if case.route == 'wgrad':
        lo, hi = t['lo'].astype(f64), t['hi'].astype(f64)
        lo[full:], hi[full:] = 0.0, 0.0
        return maps_numpy(case, t, hi=hi, lo=lo)
    out = maps_numpy(case, t)
    out[case.route][full:] = 0.0
    return out


def _wrong_partial_tile_first_image(case, t):   # wgrad: the images past the batch are read at the clamped index (image 0), not as zeros
    la = launch(case.route, case.lo, t['n'])
    extra = -t['n'] % la.ti
    lo, hi = (np.concatenate([t[s].astype(f64)] + [t[s][:1].astype(f64)] * extra) for s in ('lo', 'hi'))
    return maps_numpy(case, dict(t, n=t['n'] + extra), hi=hi, lo=lo)


def _wrong_edge(case, t):                 # a tap outside the image reads the adjacent pixel instead of the zero pixel
    return maps_numpy(case, t, mode='edge')


def _wrong_no_lh(case, t):                # one of the three partial products (l h') is missing
    return model(case, t, drop_lh=True)


def _wrong_overwrite(case, t):            # the slab reduction stores the gradient instead of adding it
    return maps_numpy(case._replace(accumulate=False), t)


def _wrong_scale_tail(case, t):           # the operand's scale is taken without the last block of the tensor
    return model(case, t, tail_missed=True)


def _wrong_relu_first(case, t):           # the ReLU is applied before the bias
    pre = maps_numpy(case._replace(bias=False, act='none'), t)[case.route]
    return {case.route: np.maximum(pre, 0) + t['b'].astype(f64)}


_whole_images = lambda c: _conv32(c) and launch(c.route, c.lo, batch(c)).ti > 1
# name -> (builder, the cases it applies to, the cases among them that reach its edge: it fails exactly those)
WRONG_KERNELS = {
    'a: tiles past the first pass missing': (_wrong_first_tile_only, lambda c: _conv32(c) and c.kernel not in (W16, W8),
                                             lambda c: launch(c.route, c.lo, batch(c)).per_wg > 1),
    'b: the images of a last partial tile dropped': (_wrong_partial_tile_dropped, _whole_images,
                                                     lambda c: batch(c) % launch(c.route, c.lo, batch(c)).ti != 0),
    'c: wgrad, a partial tile filled from the first image instead of zeros': (_wrong_partial_tile_first_image, lambda c: c.kernel == W4,
                                                                              lambda c: batch(c) % 4 != 0),
    'd: the adjacent pixel for a tap outside the image': (_wrong_edge, _conv32, lambda c: True),
    'e: the partial product l h\' missing': (_wrong_no_lh, _conv32, lambda c: True),
    'f: wgrad overwrites dwt': (_wrong_overwrite, lambda c: _conv32(c) and c.route == 'wgrad', lambda c: c.accumulate),
    'g: operand scale without the tensor\'s last 16 bytes': (_wrong_scale_tail, _conv32, lambda c: c.amax_tail is not None),
    'h: ReLU before the bias': (_wrong_relu_first, lambda c: _forward(c) and c.act == 'relu' and c.bias, lambda c: True),
}


def wrong_kernel(name, case, t):
    return _f32(WRONG_KERNELS[name][0](case, t))

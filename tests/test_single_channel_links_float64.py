"""The single-channel links -- the first encoder layer and the last decoder layer of both image models -- against float64, one kernel
at a time through the per-layer C-ABI (ops.link_down / link_up / link_wgrad, raw launches, linear maps only: no activation can flip
sides).  Needs a real MI355X.

The tables, both float64 references, the fp32 yardstick and the bar are in single_channel_cases.py; test_single_channel_cases.py
proves on the CPU that the references agree and that the table is sharp (thirteen wrong kernels fail exactly the cases that reach
their edge).  Bar: every tensor e_hip <= R * e_cpu + FLOOR (R = 4, FLOOR = 1e-7, relative L2 distances to float64); the single-channel
bias sum db2, one number, |hip - ref| <= max(R |cpu - ref|, 1e-5 |ref|).  Each case prints its figures.

Beyond the bar: every forward output is written into a view cut from a larger buffer of NaN sentinels, and the bands before and after
it must come back untouched (a persistent loop that stores one row or tile past the end lands there); every output is finite; the
three largest cases run twice and are bit-equal (the reductions are fixed-order); a weight gradient into a non-zero dw / db
accumulates.

Case -> kernel (the *_fits predicates of conv_c1.hip and link_gemm.hip; confirmed once with a kernel trace of this file, rocprofv3
--kernel-trace, a marker launch between the cases).  cus = multi_processor_count, 256 on the MI355X:

  64 x 64 <-> 32 x 32 x 32, k4 s2 p1 (conv_c1_fits)
    link_down n 1, 3, 129; n 3 with hi = (g, y, ReLU)        down_c1s_kernel<0>: 129 x 32 = 4128 rows > 1024 workgroups x 4 waves
    link_up   n 1, 3, cus + 1                                up_c1_kernel<0, false>: 2 cus + 2 tiles on 2 cus workgroups
    link_wgrad n 1, 3, 64, 65, 130; lo or hi = (g, y, ReLU)  wgrad_c1s_kernel + slab_reduce_kernel: 256 groups x 8 waves = 2048 rows
    link_up   n 3 with lo = (g, y, ReLU)                     link_gemm_kernel<4, 1, UpPolicy> (outside the route: generic)
  1 -> 64 down (single_channel_mfma_fits)                    down_single_channel_mfma_kernel
    28 -> 25 n 1, 5; output keep-mask; hi = (g, y, SELU, keep-mask); 33 -> 30 (1089 pixels); 64 -> 32 s2 p1; 14 -> 14 k3 p1;
    10 x 31 -> 7 x 28
    19 -> 16 with 16 channels                                link_gemm_kernel<4, 1, DownPolicy> (generic)
  -> 1 up
    clo 64: 25 -> 28 n 1, 4; keep-mask; 14 -> 17             up_single_channel_mfma_kernel<4>
    clo 32: 16 -> 32 s2 p1; 12 -> 15                         up_single_channel_mfma_kernel<2>
    clo 16 (19 -> 22), clo 8 (9 -> 12), clo 64 at 39 -> 42   up_single_channel_kernel (the last: T would need 103 KB of LDS)
  1 <-> 64 s1 weight gradient (conv_c1w_fits)                wgrad_c1w_kernel + slab_reduce_kernel
    28 -> 25 n 1, 5, 82; lo = (g, y, SELU, keep-mask); hi = (g, y, ReLU); 31 -> 28; 7 -> 4; 4 -> 1; 10 x 31 -> 7 x 28; 31 x 10 -> 28 x 7
    32 -> 29                                                 link_gemm_kernel<2, 2, WgradPolicy> + wgrad_reduce_kernel + channel sums

Measured on the MI355X: all 47 tests hold on the kernels as they were, 3.9 s for the file; e_hip / e_cpu 0.06 - 1.5 everywhere but
up_single_channel_kernel (one fma chain over 16 taps x clo: 1.75 - 2.03, at most 0.47 of its bar).  Figures per kernel: DESIGN.md
section 4, item 59.

Out of reach of the per-layer entry points, and so of this file: the gated down_c1s_kernel<1 / 2>, down_c1s_prep_kernel, pair_c1_kernel,
up_c1_kernel<., true>, Operand::scale and the AMAX publication."""
import numpy as np
import pytest
import torch

import single_channel_cases as sc
from test_split_kernels_float64 import _hold                 # the bar on tensors, shared with the split-operand kernels' test

pytestmark = pytest.mark.gpu

CASES = {sc.case_id(c): c for c in sc.CASES}
GUARD = 8192                                                  # floats of sentinel on each side of a forward output
SENTINEL_BITS = 0x7fc00000                                    # torch's float('nan')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _maps_hip(dev, case, t, start=None):
    """the case's maps through the raw launches, one synchronisation; start: (dw, db1, db2) to accumulate into instead of zeros"""
    from arvae_amd import ops
    g, n = case.geom, t['n']
    link = ops.Link(g.hh, g.hw, 1, g.lh, g.lw, g.clo, g.k, g.k, g.s, g.p)
    d = {k: torch.from_numpy(v).to(dev) for k, v in t.items() if isinstance(v, np.ndarray)}

    def op(side):
        if case.fold is not None and case.fold[0] == side:
            return ops._operand(d[side], d[f'y_{side}'], d.get(f'm_{side}'), case.fold[1])
        return ops._operand(d[side])
    out = {}
    if case.route in ('down', 'up'):
        shape = link.lo_shape(n) if case.route == 'down' else link.hi_shape(n)
        numel = int(np.prod(shape))
        buf = torch.full((GUARD + numel + GUARD,), float('nan'), device=dev)
        view = buf[GUARD:GUARD + numel].view(shape)
        if case.route == 'down':
            ops.link_down(link, n, op('hi'), d['w'], d['b_lo'] if case.bias else None, ops.ACT_NONE, d.get('m_out'), out=view)
        else:
            ops.link_up(link, n, op('lo'), d['w'], d['b_hi'] if case.bias else None, ops.ACT_NONE, d.get('m_out'), out=view)
        torch.cuda.synchronize()
        bands = torch.cat([buf[:GUARD], buf[GUARD + numel:]]).view(torch.int32)
        assert bool((bands == SENTINEL_BITS).all()), f'{sc.case_id(case)}: a store outside the output'
        out[case.route] = view.cpu().numpy()
        return out
    for side in (1, 2):
        dw = torch.zeros_like(d['w']) if start is None else torch.from_numpy(start[0]).to(dev)
        db = torch.zeros(g.clo if side == 1 else 1, device=dev) if start is None else torch.from_numpy(np.atleast_1d(start[side])).to(dev)
        ops.link_wgrad(link, n, op('lo'), op('hi'), dw, db, side)
        out[f'dw{side}'], out[f'db{side}'] = dw, db
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['db2'] = out['db2'].reshape(())
    return out


def _with_both_dw(maps):
    """the references hold one dW; the HIP side computes it once per bias side"""
    maps = dict(maps)
    dw = maps.pop('dw', None)
    if dw is not None:
        maps['dw1'] = maps['dw2'] = dw
    return maps


def _check(cid, got, cpu, ref):
    """tensors through the split test's _hold, the 0-d bias sum through the scalar rule of loss_cases.hold"""
    for k in got:
        assert np.all(np.isfinite(got[k])), (cid, k)
    tensors = [k for k in ref if np.ndim(ref[k]) > 0]
    _hold(cid, {k: got[k] for k in tensors}, cpu, ref)
    scalars = {k: ref[k] for k in ref if np.ndim(ref[k]) == 0}
    bad = sc.hold(cid, got, cpu, scalars)
    assert not bad, (cid, bad)


@pytest.mark.parametrize('cid', list(CASES))
def test_single_channel_link_vs_float64(dev, cus, cid):
    case = CASES[cid]
    t = sc.inputs(case, cus)
    got = _maps_hip(dev, case, t)
    if case.repeat:
        again = _maps_hip(dev, case, t)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), f'{cid} {k}: two runs differ'
    cpu, ref = (_with_both_dw(sc.maps_torch(case, t, dt)) for dt in (torch.float32, torch.float64))
    assert set(got) == set(ref)
    _check(cid, got, cpu, ref)


@pytest.mark.parametrize('cid', ['wgrad-64to32c32k4s2p1-n3', 'wgrad-28to25c64k4s1p0-n5'])
def test_weight_gradient_accumulates(dev, cus, cid):
    """link_wgrad adds to dw and db: from a non-zero start of the gradient's own size, result - start is held to the bar.  The
    yardstick does the same in fp32: its result is fp32(start + dW) - start."""
    case = CASES[cid]
    t = sc.inputs(case, cus)
    cpu, ref = (sc.maps_torch(case, t, dt) for dt in (torch.float32, torch.float64))
    rs = np.random.RandomState(11)
    start = {k: (rs.standard_normal(np.shape(v)) * np.sqrt(np.mean(np.square(v)))).astype(np.float32) for k, v in ref.items()}
    got = _maps_hip(dev, case, t, start=(start['dw'], start['db1'], start['db2']))
    start, cpu, ref = _with_both_dw(start), _with_both_dw(cpu), _with_both_dw(ref)
    moved = {k: got[k].astype(np.float64) - start[k].astype(np.float64) for k in got}
    yard = {k: (start[k] + cpu[k]).astype(np.float32).astype(np.float64) - start[k].astype(np.float64) for k in got}
    _check(cid + ' accumulated', moved, yard, ref)

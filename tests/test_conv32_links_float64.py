"""The 32 <-> 32 channel k4 s2 p1 links -- six of the dSprites step's big launches -- against float64, one kernel at a time through
the per-layer C-ABI (ops.link_down / link_up / link_wgrad with plain operands: the EP_PLAIN and EP_RELU instantiations), at the
batches where the host code of conv32.hip changes the tiling.  Needs a real MI355X.

The tables, both float64 references, the fp32 yardstick, the CPU model and the bar are in conv32_cases.py; test_conv32_cases.py
proves on the CPU that the references agree, that every case names the kernel the host code picks, that the model of the kernels'
arithmetic passes and that eight wrong kernels fail exactly the cases that reach their edge.  Bar: every tensor
e_hip <= R * e_cpu + FLOOR (R = 4, FLOOR = 1e-7, relative L2 distances to float64), and for the forward routes the same
inequality for every image separately, with the image's own distances and norm.  Each case prints its figures.

Beyond the bar: every forward output is written into a view cut from a larger buffer of NaN sentinels, and the bands before and
after it must come back untouched (the partial tiles of these kernels are guarded by buffer-resource bounds alone: a store of an
image past the batch lands there); every value is finite; every case runs twice into fresh outputs and gives the same bits (stale
LDS or AMAX state between persistent passes would not); an accumulating weight gradient starts from non-zero dw / db and must
end at prior + gradient.

Case -> kernel, cus = multi_processor_count capped at AMAX_N / 4 as grid_for_tiles caps it (256 on the MI355X):

  link_down 16 x 16   n 1, 3, cus/4, cus/4 + 1, cus/2 + 2 (+ AMAX tail)                      down32p_kernel<16>   4 n tiles
  link_down 8 x 8     n 1, 3, cus, cus + 1                                                   down32p_kernel<8>    n tiles
  link_down 4 x 4     n 1, 3, 4 cus, 4 cus + 1                                               down32s_kernel<4>    ceil(n / 2) tiles on <= 2 cus
  link_up 16 x 16     n 1, 3, cus/2, cus/2 + 1                                               up32p_kernel         2 n tiles
  link_up 8 x 8       n 1, 3, cus/2, cus/2 + 1, 2 cus                                        up32x_kernel<8,.,32>   2 n tiles
                      n 2 cus + 1 (+ AMAX tail), 2 cus + 2                                   up32x_kernel<8,.,128>  ceil(n / 2) tiles
  link_up 4 x 4       n 1, 3, 2 cus, 2 cus + 1, 4 cus                                        up32x_kernel<4,.,32>   ceil(n / 2) tiles
                      n 4 cus + 1, 8 cus, 8 cus + 1                                          up32x_kernel<4,.,128>  ceil(n / 8) tiles
  link_wgrad 4 x 4    n 1, 2, 3, 4, 5, 4 cus, 4 cus + 1; bias sides 0 / 1 / 2 at n 3 and 5;  wgrad32x_kernel<4> + slab_reduce_kernel
                      non-zero start; AMAX tail in lo and in hi                              ceil(n / 4) tiles
  link_wgrad 16 / 8   bias side 0 at n 3, 37; non-zero start at n 3                          wgrad32r_kernel<16 / 8> + slab_reduce_kernel
  outside             keep-mask; (g, y, ReLU) on either side; SELU; lo size 2                link_gemm_kernel (generic)

Measured on the MI355X: all 64 tests hold on the kernels as they were, 5.4 s for the file, the slowest test 0.8 s; e_hip / e_cpu
0.31 - 0.42 (down), 0.75 - 0.98 (up), dW 0.17 - 1.64 and bias sums 0.82 - 1.74 (weight gradients), 0.69 - 1.34 (generic); no tensor
above 0.29 of its bar, no image above 0.24.  Figures per kernel: DESIGN.md section 4, item 63.

Out of reach of the per-layer entry points, and so of this file: the gated epilogues (EP_GATE_F, EP_GATE_B),
the sign-bit outputs, chain_down_kernel, the pair* kernels, up32x_reg_kernel."""
import numpy as np
import pytest
import torch

import conv32_cases as cc

pytestmark = pytest.mark.gpu

CASES = {cc.case_id(c): c for c in cc.CASES}
GUARD = 8192                                                  # floats of sentinel on each side of a forward output
SENTINEL_BITS = 0x7fc00000                                    # torch's float('nan')
ACT = {'none': 0, 'relu': 1, 'selu': 2}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return min(torch.cuda.get_device_properties(dev).multi_processor_count, cc.AMAX_N // 4)


def _maps_hip(dev, case, t):
    """the case's maps through the raw launches into fresh outputs, one synchronisation"""
    from arvae_amd import ops
    n, lo = t['n'], case.lo
    link = ops.Link(2 * lo, 2 * lo, cc.C, lo, lo, cc.C, 4, 4, 2, 1)
    d = {k: torch.from_numpy(v).to(dev) for k, v in t.items() if isinstance(v, np.ndarray)}

    def op(side):
        if case.outside == f'fold_{side}':
            return ops._operand(d[side], d[f'y_{side}'], None, ops.ACT_RELU)
        return ops._operand(d[side])
    if case.route == 'wgrad':
        dw = d['dw0'].clone() if case.accumulate else torch.zeros_like(d['w'])
        db = None if not case.bias_side else d['db0'].clone() if case.accumulate else torch.zeros(cc.C, device=dev)
        ops.link_wgrad(link, n, op('lo'), op('hi'), dw, db, case.bias_side)
        torch.cuda.synchronize()
        out = dict(dw=dw.cpu().numpy())
        if case.bias_side:
            out['db'] = db.cpu().numpy()
        return out
    shape = link.lo_shape(n) if case.route == 'down' else link.hi_shape(n)
    numel = int(np.prod(shape))
    buf = torch.full((GUARD + numel + GUARD,), float('nan'), device=dev)
    view = buf[GUARD:GUARD + numel].view(shape)
    bias = d['b'] if case.bias else None
    if case.route == 'down':
        ops.link_down(link, n, op('hi'), d['w'], bias, ACT[case.act], d.get('m_out'), out=view)
    else:
        ops.link_up(link, n, op('lo'), d['w'], bias, ACT[case.act], d.get('m_out'), out=view)
    torch.cuda.synchronize()
    bands = torch.cat([buf[:GUARD], buf[GUARD + numel:]]).view(torch.int32)
    assert bool((bands == SENTINEL_BITS).all()), f'{cc.case_id(case)}: a store outside the output'
    return {case.route: view.cpu().numpy()}


@pytest.mark.parametrize('cid', list(CASES))
def test_conv32_link_vs_float64(dev, cus, cid):
    case = CASES[cid]
    t = cc.inputs(case, cus)
    got = _maps_hip(dev, case, t)
    again = _maps_hip(dev, case, t)
    assert set(got) == set(cc.wants(case))
    for k in got:
        assert np.all(np.isfinite(got[k])), (cid, k)
        assert got[k].tobytes() == again[k].tobytes(), f'{cid} {k}: two runs differ'
    cpu, ref = (cc.maps_torch(case, t, dt) for dt in (torch.float32, torch.float64))
    bad = cc.hold(cid, got, cpu, ref)
    assert not bad, (cid, bad)

"""CPU proof for the float64 tests of the single-channel links (single_channel_cases.py, test_single_channel_links_float64.py):

  1. the two float64 references (torch, and numpy by explicit patches) agree to 1e-12 relative at every case, and with the layers
     of oracle/image_vae.py where the oracle has them: dSprites conv1 and deconv4, Morpho-MNIST's first and last layer;
  2. the fp32 yardstick passes the bar at every case, and every 0-d output (the single-channel bias sum) has a reference of at least a
     tenth of sqrt(count) x rms, so that the scalar bar never rests on a sum that happened to cancel;
  3. an fp32 numpy restatement of each streaming weight gradient's own summation order passes the bar at every case (figures printed);
  4. the table is sharp: every wrong kernel of WRONG_KERNELS fails the bar at each case that reaches its edge and passes the cases of
     the same kernel that do not.  That second half is what shows the large batches and the odd geometries are needed.

Runs anywhere (no GPU)."""
from unittest import mock

import numpy as np
import pytest
import torch

import single_channel_cases as sc
from oracle import image_vae

CASES = {sc.case_id(c): c for c in sc.CASES}


def _quiet(*_a):
    pass


@pytest.fixture(scope='module')
def computed():
    """inputs and the three results of a case, computed once and kept while consecutive tests ask for the same case"""
    last = {}

    def get(cid):
        if last.get('id') != cid:
            last.clear()
            case = CASES[cid]
            t = sc.inputs(case)
            last.update(id=cid, case=case, t=t, ref=sc.maps_torch(case, t, torch.float64), cpu=sc.maps_torch(case, t, torch.float32))
        return last['case'], last['t'], last['ref'], last['cpu']
    return get


# ---------------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize('cid', list(CASES))
def test_references_agree_and_the_yardstick_passes(computed, cid):
    case, t, ref, cpu = computed(cid)
    other = sc.maps_numpy(case, t)
    assert set(ref) == set(other) == set(sc.wants(case))
    for k in ref:
        assert ref[k].shape == np.shape(other[k]) and ref[k].dtype == np.float64, k
        assert sc.rel(other[k], ref[k]) <= 1e-12, (k, sc.rel(other[k], ref[k]))
    assert not sc.hold(cid, cpu, cpu, ref, say=_quiet)
    margin = sc.scalar_margin(case, t)
    assert (margin is None) == (not any(np.ndim(v) == 0 for v in ref.values()))
    if margin is not None:
        assert margin >= 0.1, f'{cid}: the bias sum cancelled ({margin:.3f} of sqrt(count) x rms): set a SEED_SALT'


class _Recorder:
    """torch.nn.functional with every conv2d / conv_transpose2d call recorded"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(torch.nn.functional, name)
        if name not in ('conv2d', 'conv_transpose2d'):
            return fn

        def rec(x, w, b=None, **kw):
            y = fn(x, w, b, **kw)
            self.calls.append((name, x, w, b, y))
            return y
        return rec


@pytest.mark.parametrize('kind,g', [('dsprites', sc.G_DS), ('mnist', sc.G_MN)])
def test_references_are_the_oracles_first_and_last_layer(kind, g):
    """encode / decode of oracle/image_vae.py in float64 with every convolution call recorded: the first call of the encoder and the
    last of the decoder, on the operands the oracle gave them, are what both references compute for that geometry"""
    rs = np.random.RandomState(7)
    p = {k: torch.from_numpy(rs.standard_normal(s) * 0.1) for k, s in image_vae.SHAPES[kind].items()}
    n = 2
    x = torch.from_numpy(rs.random_sample((n, 1, g.hh, g.hw)))
    z = torch.from_numpy(rs.standard_normal((n, image_vae.Z_DIM[kind])))
    rec = _Recorder()
    with mock.patch.object(image_vae, 'F', rec):
        image_vae.encode(kind, p, x)
        first = rec.calls[0]
        image_vae.decode(kind, p, z)
        last = rec.calls[-1]
    assert first[0] == 'conv2d' and last[0] == 'conv_transpose2d'
    nhwc = lambda a: a.detach().permute(0, 2, 3, 1).contiguous()
    for route, (_name, src, w, b, y) in (('down', first), ('up', last)):
        case = sc._c(route, g, n, 'oracle', 'oracle')
        assert tuple(w.shape) == (g.clo, 1, g.k, g.k)
        t = dict(n=n, w=w.numpy(), b_lo=b.numpy(), b_hi=b.numpy())           # (float64 data: the references convert, they do not round)
        side = 'hi' if route == 'down' else 'lo'
        t[side] = nhwc(src).numpy()
        for got in (sc.maps_torch(case, t, torch.float64), sc.maps_numpy(case, t)):
            assert got[route].shape == tuple(nhwc(y).shape)
            assert sc.rel(got[route], nhwc(y).numpy()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- 3. streaming order
STREAMED = [cid for cid, c in CASES.items() if c.kernel in ('wgrad_c1s_kernel', sc.C1W)]


@pytest.mark.parametrize('cid', STREAMED)
def test_the_streaming_summation_order_passes(computed, cid):
    case, t, ref, cpu = computed(cid)
    got = sc.wgrad_stream(case, t)
    print(f'{cid} dw: restatement {sc.rel(got["dw"], ref["dw"]):.2e}  torch fp32 {sc.rel(cpu["dw"], ref["dw"]):.2e}  '
          f'bar {sc.R * sc.rel(cpu["dw"], ref["dw"]) + sc.FLOOR:.2e}')
    bad = sc.hold(cid, got, cpu, ref)
    assert not bad, (cid, bad)


# ---------------------------------------------------------------------------------------------------------------- 4. sharpness
def test_every_wrong_kernel_has_cases_on_both_sides():
    """statically: each defect applies somewhere and reaches its edge somewhere; (a), (e), (f), (i), (j), the ones with an edge the
    small cases do not reach, also have a case that stays inside"""
    for name, (_fn, applies, reaches) in sc.WRONG_KERNELS.items():
        mine = [c for c in sc.CASES if applies(c)]
        assert any(reaches(c) for c in mine), name
        if name[0] in 'aefij':
            assert any(not reaches(c) for c in mine), name
    reach = lambda letter: {sc.case_id(c) for name, (_f, a, r) in sc.WRONG_KERNELS.items() if name[0] == letter for c in sc.CASES if a(c) and r(c)}
    assert reach('a') == {'down-64to32c32k4s2p1-n129'}
    assert reach('e') == {'up-64to32c32k4s2p1-ncus+1'}
    assert {sc.batch(CASES[c]) for c in reach('f')} == {65, 130}
    assert all(CASES[c].geom.lw in (25, 28) for c in reach('i'))
    assert 'down-64to32c64k4s2p1-n2' not in reach('j') and 'down-14to14c64k3s1p1-n3' in reach('j') and 'down-28to25c64k4s1p0-n5' in reach('j')


@pytest.mark.parametrize('cid', [cid for cid, c in CASES.items() if any(a(c) for _f, a, _r in sc.WRONG_KERNELS.values())])
def test_wrong_kernels_fail_exactly_where_their_edge_is_reached(computed, cid):
    case, t, ref, cpu = computed(cid)
    for name, (_fn, applies, reaches) in sc.WRONG_KERNELS.items():
        if not applies(case):
            continue
        bad = sc.hold(f'{cid} [{name}]', sc.wrong_kernel(name, case, t), cpu, ref)
        assert bool(bad) == bool(reaches(case)), (cid, name, 'fails' if bad else 'passes', bad)


def test_dropped_rows_move_the_weight_gradient_by_what_the_issue_measured():
    """the size of what the large batches see: without the rows past the first pass dW of the dSprites geometry is 0.12 off at
    n = 65 and 0.68 at n = 130 (relative L2)"""
    for n, lo, hi in ((65, 0.08, 0.2), (130, 0.55, 0.8)):
        case = next(c for c in sc.C1_CASES if c.route == 'wgrad' and c.n == n and c.fold is None)
        t = sc.inputs(case)
        e = sc.rel(sc.wrong_kernel('f: wgrad c1s, second pass missing', case, t)['dw'], sc.maps_numpy(case, t)['dw'])
        print(f'n = {n}: dW without the second pass is {e:.3f} off')
        assert lo < e < hi

"""The kernels around the GRU recurrences at the row widths the 256- and 512-wide sequence path feeds them: 3H and 6H floats per
row (768 to 3072), where their own suites stop at 768.  Needs a real MI355X.

  the lookup ops.embed(..., time_major=True) and its wide-row segment sum at 6 x 256 and 6 x 512 columns (the encoder's projection
  table, Encoder._first_layer_by_lookup), ops.tick_input_projection at 3 x 256 and 3 x 512 (the tick RNN's first layer), and
  ops.dense_pair at 6 x 256 and 6 x 512 output columns (both directions' input projections as one product; layer 0 over the 35
  table rows, layer 1 over steps x batch rows of 2H inputs) with the weight gradients of link_wgrad behind it.

Generators, float64 references, fp32 CPU yardsticks and the bar (loss_cases.hold: e_got <= R * e_cpu + FLOOR) are those of
sequence_cases.py; batches of 5 and 21 measures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sequence_cases as sc

pytestmark = pytest.mark.gpu

HIDDEN = (256, 512)
MEASURES = (5, 21)
VOCAB = 35

# (dim, vocab, (batch, steps), time_major, accumulate, pattern): sequence_cases.EMBED_CASES' form
EMBED_WIDE = [(6 * 256, VOCAB, (5, 24), 1, 0, 'uniform'), (6 * 256, VOCAB, (21, 24), 1, 1, 'out_of_range'),
              (6 * 512, VOCAB, (5, 24), 1, 1, 'uniform'), (6 * 512, VOCAB, (21, 24), 1, 0, 'missing')]
# (hidden, batch, vocab, preset): sequence_cases.TICK_PROJECTION_CASES' form
PROJECTION_WIDE = [(256, 5, VOCAB, False), (256, 21, VOCAB, True), (512, 5, VOCAB, True), (512, 21, VOCAB, False)]
# (hidden, rows, inputs): layer 0's table product and layer 1's whole-sequence product
PAIR_WIDE = [(h, VOCAB, 10) for h in HIDDEN] + [(h, 24 * b, 2 * h) for h in HIDDEN for b in MEASURES]


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
    bad = sc.hold(sc.case_id(case), got, cpu, ref)
    assert not bad, (sc.case_id(case), bad)


@pytest.mark.parametrize('case', EMBED_WIDE, ids=sc.case_id)
def test_lookup_and_segment_sum_at_6h_columns(dev, case):
    from arvae_amd import ops
    inp = sc.embed_inputs(case)
    assert inp['dim'] > sc.NARROW_MAX and ops.segment_sum_fits(inp['vocab'], inp['batch'] * inp['steps'])
    ref, cpu = sc.embed_ref(inp), sc.embed_cpu(inp)
    idx, g = _t(inp['idx'], dev), _t(inp['g'], dev)

    def run():
        table = _t(inp['table'], dev, True)
        if inp['acc']:
            table.grad = _t(inp['old'], dev).clone()
        out = ops.embed(idx, table, time_major=True)
        assert tuple(out.shape) == (inp['steps'], inp['batch'], inp['dim'])
        out.backward(g.view(out.shape))
        used = np.zeros(inp['vocab'], bool)
        used[np.clip(inp['idx'].ravel(), 0, inp['vocab'] - 1)] = True
        return dict(x_out=_np(out).reshape(-1, inp['dim']), dtable=_np(table.grad), x_unused_rows=np.ascontiguousarray(_np(table.grad)[~used]))

    a, b = run(), run()
    _hold(case, a, cpu, ref)
    assert all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a), 'two calls differ'


@pytest.mark.parametrize('case', PROJECTION_WIDE, ids=sc.case_id)
def test_tick_input_projection_at_3h_columns(dev, case):
    from arvae_amd import ops
    inp = sc.tick_projection_inputs(case)
    ref, cpu = sc.tick_projection_ref(inp), sc.tick_projection_cpu(inp)
    batch, nb, steps, hid = inp['batch'], inp['beats'], inp['tpb'], inp['hidden']
    assert ops.segment_sum_fits(inp['vocab'] + 1, nb * steps * batch)
    p = {k: _t(inp[k], dev, True) for k in ('table', 'x0', 'beat_emb', 'w_ih', 'b_ih')}
    for k in ('table', 'x0', 'w_ih', 'b_ih'):
        if inp['preset']:
            p[k].grad = _t(inp['old_' + k], dev).clone()
    gi = ops.tick_input_projection(p['table'], p['x0'], p['beat_emb'], p['w_ih'], p['b_ih'], _t(inp['tokens'], dev), nb, steps)
    assert tuple(gi.shape) == (steps, nb * batch, 3 * hid)
    gi.backward(_t(inp['dgi'], dev).view(gi.shape))
    got = dict(gi=_np(gi).reshape(-1, 3 * hid), d_table=_np(p['table'].grad), d_x0=_np(p['x0'].grad), d_beat=_np(p['beat_emb'].grad),
               d_w=_np(p['w_ih'].grad), d_b=_np(p['b_ih'].grad))
    _hold(case, got, cpu, ref)


def _pair_inputs(case):
    hid, rows, fin = case
    rs = sc._rs('dense_pair_wide', case)
    k = 1.0 / np.sqrt(hid)
    return dict(x=rs.standard_normal((rows, fin)).astype(sc.f32), w=rs.uniform(-k, k, (6 * hid, fin)).astype(sc.f32),
                b=rs.uniform(-k, k, 6 * hid).astype(sc.f32), g=rs.standard_normal((rows, 6 * hid)).astype(sc.f32))


def _pair_torch(inp, dt):
    x, w, b = (torch.from_numpy(inp[k]).to(dt).requires_grad_(True) for k in ('x', 'w', 'b'))
    out = F.linear(x, w, b)
    out.backward(torch.from_numpy(inp['g']).to(dt))
    return dict(out=out.detach().numpy(), dx=x.grad.numpy(), dw=w.grad.numpy(), db=b.grad.numpy())


@pytest.mark.parametrize('case', PAIR_WIDE, ids=sc.case_id)
def test_dense_pair_at_6h_columns(dev, case):
    """two (3H, in) layers back to back in one allocation, with their gradient buffers, as the trainer's arena lays them out: one
    (rows, 6H) product, its input gradient, and link_wgrad at Link.dense(in, 6H) into the adjacent gradient buffers"""
    from arvae_amd import ops
    hid, rows, fin = case
    inp = _pair_inputs(case)
    ref, cpu = _pair_torch(inp, torch.float64), _pair_torch(inp, torch.float32)
    nw, nb = 3 * hid * fin, 3 * hid
    flat, gflat = torch.empty(2 * nw + 2 * nb, device=dev), torch.zeros(2 * nw + 2 * nb, device=dev)
    flat[:2 * nw].copy_(_t(inp['w'], dev).reshape(-1))
    flat[2 * nw:].copy_(_t(inp['b'], dev))
    prm = []
    for off, shape in ((0, (3 * hid, fin)), (nw, (3 * hid, fin)), (2 * nw, (3 * hid,)), (2 * nw + nb, (3 * hid,))):
        n = int(np.prod(shape))
        p = torch.nn.Parameter(flat[off:off + n].view(shape))
        p.grad = gflat[off:off + n].view(shape)
        prm.append(p)
    wa, wb, ba, bb = prm
    xd = _t(inp['x'], dev, True)
    out = ops.dense_pair(xd, wa, ba, wb, bb)
    assert out is not None and tuple(out.shape) == (rows, 6 * hid)
    out.backward(_t(inp['g'], dev))
    got = dict(out=_np(out), dx=_np(xd.grad), dw=_np(gflat[:2 * nw].view(6 * hid, fin)), db=_np(gflat[2 * nw:]))
    _hold(case, got, cpu, ref)

"""Case table, problems and CPU reference of the tests of the streamed-weights beam search at hidden sizes 256 and 512
(ar-vae_amd/csrc/beam_wide.hip: beam_wide_l0_kernel<H>, beam_wide_l1_kernel<H>, beam_wide_logits_kernel<H>, beam_select_kernel, four
launches per tick), shared by the CPU test of the table itself (test_beam_wide_cases.py) and the GPU test (test_beam_wide_gpu.py).
No test in here.

The bars come from gru_cases.py (the output bar: logits are outputs); nothing here adds a number.

A case is (hidden, batch, vocab, width, groups, form) or (hidden, batch, vocab, width, groups, form, beats, ticks_per_beat); 4 beats x 6
ticks where the last two are left out.  Rows = batch * width; the recurrence kernels take 32 rows per workgroup in two 16-row blocks,
the logits kernel 16 rows, 16 notes a tile:
  (256, 5, 35, 4)     20 rows, under one 32-row tile; three 16-note tiles, the last ragged
  (512, 3, 70, 16)    48 rows: a code is exactly a 16-row block and the rows cross a 32-row tile; one mask for every code
  (256, 21, 128, 3)   63 rows: codes straddle the 16- and the 32-row boundaries; the full vocabulary
  (512, 11, 33, 2)    a tile boundary in the vocabulary; a plan that forces one note on every fourth tick: dead slots
  (512, 7, 35, 8, 4) and (256, 6, 20, 6, 2)   the grouped search under such a plan, penalty 0.5
  (256, 40, 2, 1)     width 1 and two notes, the smallest of both: the argmax free run
  (256, 5, 35, 4) over 2 x 3 ticks, and (512, 4, 35, 3) over 5 x 1: every tick restarts"""
import functools

import numpy as np

FORMS = ('plain', 'masked', 'planned', 'groups')
PENALTY = 0.5

CASES = [
    (256, 5, 35, 4, 1, 'plain'),
    (512, 3, 70, 16, 1, 'masked'),
    (256, 21, 128, 3, 1, 'plain'),
    (512, 11, 33, 2, 1, 'planned'),
    (512, 7, 35, 8, 4, 'groups'),
    (256, 6, 20, 6, 2, 'groups'),
    (256, 40, 2, 1, 1, 'plain'),
    (256, 5, 35, 4, 1, 'plain', 2, 3),
    (512, 4, 35, 3, 1, 'planned', 5, 1),
]


def shape(case):
    """-> (beats, ticks_per_beat) of a case"""
    return tuple(case[6:8]) if len(case) > 6 else (4, 6)


def case_id(case):
    hid, batch, vocab, width, groups, form = case[:6]
    beats, tpb = shape(case)
    return f'H{hid}-B{batch}-V{vocab}-W{width}-G{groups}-{form}-{beats}x{tpb}'


def make_plan(rs, batch, ticks, vocab):
    """a note plan (batch, ticks, vocab) uint8: every fourth tick (the first among them) forces one note, the others allow several
    (two at least)"""
    plan = (rs.uniform(size=(batch, ticks, vocab)) < 0.3).astype(np.uint8)
    for b in range(batch):
        for t in range(ticks):
            if t % 4 == 0:
                plan[b, t] = 0
                plan[b, t, rs.randint(vocab)] = 1
            else:
                plan[b, t, rs.choice(vocab, 2, replace=False)] = 1
    return plan


@functools.lru_cache(maxsize=None)
def problem(hid, batch, vocab, width, groups, form, beats=4, tpb=6):
    """seeded fp32 numpy tensors of a case, tick_wide_cases.problem's style and scales.  `parents` and `tokens` (B, ticks, W): any
    history (inside the plan or the mask where there is one), what the CPU test feeds the reference.  The returned arrays are shared
    between tests: nobody writes to them."""
    rs = np.random.RandomState(hid + 7 * batch + 13 * vocab + 31 * width + 101 * FORMS.index(form) + 1009 * groups + beats * tpb)
    k = 1.0 / np.sqrt(hid)
    ticks = beats * tpb
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                      # noqa: E731
    uni = lambda *s: f32(rs.uniform(-k, k, s))                               # noqa: E731
    p = dict(hid=hid, batch=batch, vocab=vocab, width=width, groups=groups, beats=beats, tpb=tpb, ticks=ticks, form=form,
             w_hh0=uni(3 * hid, hid), b_hh0=uni(3 * hid), w_ih1=uni(3 * hid, hid), b_ih1=uni(3 * hid), w_hh1=uni(3 * hid, hid),
             b_hh1=uni(3 * hid), w_out=f32(rs.uniform(-4 * k, 4 * k, (vocab, hid))), b_out=f32(rs.uniform(0.0, 0.6, vocab)),
             h0=f32(rs.uniform(-1.0, 1.0, (2, beats * batch, hid))), gib=f32(0.5 * rs.standard_normal((beats * batch, 3 * hid))),
             ptab=f32(0.5 * rs.standard_normal((vocab + 1, 3 * hid))), allow=None, plan=None, penalty=PENALTY,
             parents=rs.randint(0, width, (batch, ticks, width)).astype(np.int32),
             tokens=rs.randint(0, vocab, (batch, ticks, width)).astype(np.int64))
    if form == 'masked':
        allow = (rs.uniform(size=vocab) < 0.5).astype(np.uint8)
        allow[rs.choice(vocab, width + 2, replace=False)] = 1
        p['allow'] = allow
    if form in ('planned', 'groups'):
        p['plan'] = make_plan(rs, batch, ticks, vocab)
    return p


def reference_logits(p, parents, tokens, dtype):
    """the logits (B, ticks, W, V) of the decoder of problem `p` carried along the history `parents`, `tokens` (B, ticks, W), computed
    on the CPU in `dtype` (np.float64 or np.float32: every operand cast first, every product and sum in that type).  Rows are code * W +
    k; at tick t = tpb * beat + j row (code, k) takes the states of row (code, parents[code, t - 1, k]) -- the beat's initial states of
    its code at j == 0 --, layer 0 takes ptab[tokens[code, t - 1, k]] + gib[beat][code] (row V of ptab at tick 0), layer 1 layer 0's
    new state, and logits = relu(W_out h_l1 + b_out)"""
    c = lambda a: np.asarray(a, dtype)                                       # noqa: E731
    hid, batch, vocab, width, tpb = p['hid'], p['batch'], p['vocab'], p['width'], p['tpb']
    w_hh0, b_hh0, w_ih1, b_ih1, w_hh1, b_hh1, w_out, b_out = (c(p[n]) for n in ('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1',
                                                                                'w_out', 'b_out'))
    h0, gib, ptab = c(p['h0']), c(p['gib']), c(p['ptab'])
    parents, tokens = np.asarray(parents, np.int64), np.asarray(tokens, np.int64)
    one = dtype(1.0)
    code = np.repeat(np.arange(batch), width)                                # row -> code

    def cell(gi, gh, h):
        r = one / (one + np.exp(-(gi[:, :hid] + gh[:, :hid])))
        z = one / (one + np.exp(-(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])))
        n = np.tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
        return (one - z) * n + z * h

    out = np.zeros((batch, p['ticks'], width, vocab), dtype)
    a = b = None
    for t in range(p['ticks']):
        beat, j = divmod(t, tpb)
        rows = beat * batch + code
        if j == 0:
            a, b = h0[0, rows], h0[1, rows]
        else:
            src = code * width + parents[:, t - 1].reshape(-1)
            a, b = a[src], b[src]
        prev = np.full(batch * width, vocab) if t == 0 else tokens[:, t - 1].reshape(-1)
        a = cell(ptab[prev] + gib[rows], a @ w_hh0.T + b_hh0, a)
        b = cell(a @ w_ih1.T + b_ih1, b @ w_hh1.T + b_hh1, b)
        out[:, t] = np.maximum(b @ w_out.T + b_out, 0).reshape(batch, width, vocab)
    assert out.dtype == dtype
    return out

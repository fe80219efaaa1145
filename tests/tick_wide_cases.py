"""Case table, problems and CPU reference decoder of the tests of the streamed-weights free-running tick decoder at hidden sizes 256
and 512 (ar-vae_amd/csrc/tick_wide.hip: tick_wide_l0_kernel<H>, tick_wide_l1_kernel<H, MASK>, tick_wide_out_kernel<H, PICK>, three
launches per tick), shared by the CPU test of the table itself (test_tick_wide_cases.py) and the GPU test (test_tick_wide_gpu.py).
No test in here.

The bars come from gru_cases.py (the output bar: logits are outputs); nothing here adds a number.

A case is (hidden, batch, vocab, beats, ticks_per_beat, form, masked):
  batch    5 (fewer rows than any tile) and 37: 5 modulo every row-tile height the kernels are instantiated with (ROW_TILES: 32 rows
           for the two recurrence kernels, 16 for logits + pick) with at least one full tile -- gru_wide_cases.ROWS' convention
  vocab    35 (no multiple of 16: the last 16-note tile is ragged) and 70 (past the one-launch kernels' ceiling of 64; five tiles: one
           wave of the four computes two)
  shape    4 x 6 ticks (the decoder's), and 1 x 1 once: the first tick is also the last
  form     FORMS: 'argmax', 'multinomial', 'filtered' (top-k, nucleus and an allowed mask), 'planned' (draws under a note plan),
           'planned_argmax' (top_k = 1 and draws of 1 under the plan, as the decoder asks for a plan's argmax)
  masked   the training pass's keep-masks (ticks, batch, hidden) between the layers, scaled by 2; argmax and multinomial only"""
import functools

import numpy as np

HIDDEN = (256, 512)
ROW_TILES = (16, 32)                       # TW_ORT of tick_wide.hip and GWT_RT of gru_wide_tile.h
ROWS = (5, 37)                             # 37 = 2 * 16 + 5 = 32 + 5
VOCABS = (35, 70)
FORMS = ('argmax', 'multinomial', 'filtered', 'planned', 'planned_argmax')
KEEP_SCALE = 2.0                           # 1 / (1 - 0.5)
TEMPERATURE = 0.7
TOP_K, TOP_P = 6, 0.9                      # the filtered and the planned draws' cuts

CASES = [
    (256, 37, 35, 4, 6, 'argmax', False), (512, 5, 70, 4, 6, 'argmax', False),
    (256, 5, 70, 4, 6, 'argmax', True), (512, 37, 35, 4, 6, 'argmax', True),
    (256, 37, 70, 4, 6, 'multinomial', False), (512, 5, 35, 4, 6, 'multinomial', False),
    (256, 5, 35, 4, 6, 'multinomial', True), (512, 37, 70, 4, 6, 'multinomial', True),
    (256, 5, 35, 4, 6, 'filtered', False), (512, 37, 70, 4, 6, 'filtered', False),
    (256, 37, 70, 4, 6, 'planned', False), (512, 5, 35, 4, 6, 'planned', False),
    (256, 5, 35, 4, 6, 'planned_argmax', False), (512, 37, 70, 4, 6, 'planned_argmax', False),
    (256, 5, 35, 1, 1, 'argmax', False),
]


def case_id(case):
    hid, batch, vocab, beats, tpb, form, masked = case
    return f'H{hid}-B{batch}-V{vocab}-{beats}x{tpb}-{form}{"-masked" if masked else ""}'


def make_plan(rs, batch, ticks, vocab):
    """a note plan (batch, ticks, vocab) uint8 with the three kinds of tick: every third tick forces one note, the others allow several
    (two at least), and row min(1, batch - 1) allows none at its tick ticks // 2"""
    plan = (rs.uniform(size=(batch, ticks, vocab)) < 0.3).astype(np.uint8)
    for b in range(batch):
        for t in range(ticks):
            if t % 3 == 0:
                plan[b, t] = 0
                plan[b, t, rs.randint(vocab)] = 1
            else:
                plan[b, t, rs.choice(vocab, 2, replace=False)] = 1
    plan[min(1, batch - 1), ticks // 2] = 0
    return plan


def plan_kinds(plan):
    """-> (ticks with exactly one allowed note, ticks with several, ticks with none), counted over all rows"""
    n = plan.astype(np.int64).sum(-1)
    return int((n == 1).sum()), int((n > 1).sum()), int((n == 0).sum())


@functools.lru_cache(maxsize=None)
def problem(hid, batch, vocab, beats, tpb, form, masked):
    """seeded fp32 numpy tensors of a case, gru_cases.problem's style: recurrent weights and biases uniform in [-k, k], k = 1/sqrt(H);
    the note projection four times as wide with a positive bias (the logits are ReLU outputs: most stay above zero and apart);
    initial states uniform in [-1, 1]; gib and ptab normal.  The returned arrays are shared between tests: nobody writes to them."""
    rs = np.random.RandomState(hid + 7 * batch + 13 * vocab + 101 * FORMS.index(form) + (1000 if masked else 0) + beats * tpb)
    k = 1.0 / np.sqrt(hid)
    ticks = beats * tpb
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                      # noqa: E731
    uni = lambda *s: f32(rs.uniform(-k, k, s))                               # noqa: E731
    p = dict(hid=hid, batch=batch, vocab=vocab, beats=beats, tpb=tpb, ticks=ticks, form=form,
             w_hh0=uni(3 * hid, hid), b_hh0=uni(3 * hid), w_ih1=uni(3 * hid, hid), b_ih1=uni(3 * hid), w_hh1=uni(3 * hid, hid),
             b_hh1=uni(3 * hid), w_out=f32(rs.uniform(-4 * k, 4 * k, (vocab, hid))), b_out=f32(rs.uniform(0.0, 0.6, vocab)),
             h0=f32(rs.uniform(-1.0, 1.0, (2, beats * batch, hid))), gib=f32(0.5 * rs.standard_normal((beats * batch, 3 * hid))),
             ptab=f32(0.5 * rs.standard_normal((vocab + 1, 3 * hid))),
             mask=(rs.uniform(size=(ticks, batch, hid)) >= 0.5).astype(np.uint8) if masked else None, keep_scale=KEEP_SCALE,
             uniforms=None, temperature=1.0, top_k=None, top_p=None, allow=None, plan=None,
             tokens=rs.randint(0, vocab, (batch, ticks)).astype(np.int64))   # any notes: what the CPU test feeds the reference
    if form != 'argmax':
        p['uniforms'] = f32(1.0 - rs.uniform(size=(batch, ticks)))           # (0, 1]
        p['temperature'] = TEMPERATURE
    if form == 'filtered':
        allow = (rs.uniform(size=vocab) < 0.7).astype(np.uint8)
        allow[rs.choice(vocab, TOP_K + 2, replace=False)] = 1
        p.update(top_k=TOP_K, top_p=TOP_P, allow=allow)
    if form in ('planned', 'planned_argmax'):
        p['plan'] = make_plan(rs, batch, ticks, vocab)
        if form == 'planned':
            p.update(top_k=TOP_K, top_p=TOP_P)
        else:
            p.update(top_k=1, uniforms=np.ones((batch, ticks), np.float32))
    return p


def reference_logits(p, tokens, dtype):
    """the logits (B, ticks, V) of the decoder of problem `p` fed `tokens` (B, ticks), computed on the CPU in `dtype` (np.float64 or
    np.float32: every operand cast first, every product and sum in that type): at tick t = tpb * beat + j layer 0 takes
    ptab[previous note] + gib[beat] (row V of ptab at tick 0), the states restart from h0 at j == 0, layer 1 takes layer 0's new
    state times keep-mask times keep_scale, and logits = relu(W_out h_l1 + b_out)"""
    c = lambda a: np.asarray(a, dtype)                                       # noqa: E731
    hid, batch, vocab, tpb = p['hid'], p['batch'], p['vocab'], p['tpb']
    w_hh0, b_hh0, w_ih1, b_ih1, w_hh1, b_hh1, w_out, b_out = (c(p[n]) for n in ('w_hh0', 'b_hh0', 'w_ih1', 'b_ih1', 'w_hh1', 'b_hh1',
                                                                                'w_out', 'b_out'))
    h0, gib, ptab = c(p['h0']), c(p['gib']), c(p['ptab'])
    one = dtype(1.0)

    def cell(gi, gh, h):
        r = one / (one + np.exp(-(gi[:, :hid] + gh[:, :hid])))
        z = one / (one + np.exp(-(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])))
        n = np.tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
        return (one - z) * n + z * h

    out = np.zeros((batch, p['ticks'], vocab), dtype)
    a = b = None
    for t in range(p['ticks']):
        beat, j = divmod(t, tpb)
        rows = slice(beat * batch, (beat + 1) * batch)
        if j == 0:
            a, b = h0[0, rows], h0[1, rows]
        prev = np.full(batch, vocab) if t == 0 else np.asarray(tokens)[:, t - 1]
        a = cell(ptab[prev] + gib[rows], a @ w_hh0.T + b_hh0, a)
        x = a if p['mask'] is None else a * (c(p['mask'][t]) * dtype(p['keep_scale']))
        b = cell(x @ w_ih1.T + b_ih1, b @ w_hh1.T + b_hh1, b)
        out[:, t] = np.maximum(b @ w_out.T + b_out, 0)
    assert out.dtype == dtype
    return out

"""Case tables, float64 references, fp32 CPU yardsticks and restatements for the float64 tests of the MeasureVAE kernels that are not
GEMMs (ar-vae_amd/csrc/sequence.hip, attributes.h): the embedding lookup and its segment-sum gradient (narrow and wide rows), the
re-associated layer-0 input projection of the tick RNN (tick_rows, tick_gi, and the composite ops.tick_input_projection), the
column concat / split, scale_mask, broadcast_rows and GRU gate kernels, and the measure attribute labels.  Shared by the GPU test
(test_sequence_kernels_float64.py) and by the CPU test that proves the references right and the bar discriminating
(test_sequence_cases.py).  No test in here.

Per family, as in loss_cases.py:  <family>_CASES, <family>_inputs(case) (seeded by the case), <family>_ref(inp) (float64 numpy),
<family>_cpu(inp) (torch CPU fp32: index_add_ / indexing for the sums, F.linear for the composite), <family>_chain(inp, wrong)
(the kernel's DOCUMENTED summation order in plain fp32 numpy; `wrong` names one planted defect of WRONG_KERNELS).
The bar is loss_cases.hold(): 'x_*' bit-equal, 'n_*' exact, tensors e_got <= R * e_cpu + FLOOR.

Segment lengths: the longest sums any case forms are 2064 terms (one_token at 86 x 24 positions) and, in the one tick_gi case past
the grid cap, the 5500 tick-0 rows of x_0: within the few thousand terms up to which split_cases.py found a correct fp32 order
separable from a wrong result."""
import numpy as np
import torch
import torch.nn.functional as F

from loss_cases import FLOOR, R, _rs, case_id, f32, f64, hold, rel            # noqa: F401  (the bar is imported, never redefined)

EMBED_POS, EMBED_WSPLIT, EMBED_WLANES = 64, 16, 8           # sequence.hip
GRID_CAP = 2048 * 256                                       # blocks_for(): more elements than this go round the grid-stride loop twice
NARROW_MAX = 128                                            # dim <= 128: embed_bwd_partial_kernel, above: embed_bwd_wide_kernel


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def seq_sum0(x):
    """fp32 sum along axis 0 in index order (np.cumsum adds sequentially); an empty axis sums to 0"""
    x = np.asarray(x, f32)
    return np.cumsum(x, 0, dtype=f32)[-1] if x.shape[0] else np.zeros(x.shape[1:], f32)


def tokens_for(rs, pattern, vocab, shape):
    """int64 tokens: uniform | one_token (the longest segment) | missing (odd tokens never occur) | out_of_range (-1, -7, vocab,
    vocab + 5 and 2**32 + 3 planted among valid tokens)"""
    n = int(np.prod(shape))
    if pattern == 'one_token':
        tok = np.full(n, min(2, vocab - 1))
    elif pattern == 'missing':
        tok = 2 * rs.randint(0, (vocab + 1) // 2, n)
    else:
        tok = rs.randint(0, vocab, n)
    tok = tok.astype(np.int64)
    if pattern == 'out_of_range':
        bad = [-1, -7, vocab, vocab + 5, 2 ** 32 + 3]
        at = rs.permutation(n)[:len(bad)]
        tok[at] = bad[:len(at)]
    return tok.reshape(shape)


def _lane4(parts):
    """embed_bwd_reduce_kernel: lane q of four adds partials q, q + 4, ... in order; (lane 0 + lane 1) + (lane 2 + lane 3)"""
    s = [seq_sum0(parts[q::4]) for q in range(4)]
    return (s[0] + s[1]) + (s[2] + s[3])


def segment_sums(gpos, tok, nv, wide, wrong=None):
    """sum of the gradient rows gpos [n][dim] (position order) per token tok [n] -> [nv][dim], in the kernels' documented fp32 order.
    narrow: blocks of EMBED_POS positions, each summed in position order; wide: EMBED_WSPLIT position groups of ceil(n / 16), lane pl
    of eight adds positions pl, pl + 8, ... in order, the lanes are added in lane order; either way the partials go through _lane4.
    A token < 0 or >= nv matches no row (what an unclamped index does in the narrow kernel)."""
    n, dim = gpos.shape
    out = np.zeros((nv, dim), f32)
    if wide:
        per = (n + EMBED_WSPLIT - 1) // EMBED_WSPLIT
        groups = [(g * per, min(g * per + per, n)) for g in range(EMBED_WSPLIT)]
        if wrong == 'last position group dropped':
            last = max(g for g, (lo, hi) in enumerate(groups) if hi > lo)
            groups[last] = (0, 0)
    else:
        blocks = (n + EMBED_POS - 1) // EMBED_POS
        groups = [(z * EMBED_POS, min(z * EMBED_POS + EMBED_POS, n)) for z in range(blocks)]
        if wrong == 'last partial block dropped' and n % EMBED_POS:
            groups[-1] = (0, 0)
    for v in np.unique(tok):
        if v < 0 or v >= nv:
            continue
        parts = np.zeros((len(groups), dim), f32)
        for k, (lo, hi) in enumerate(groups):
            m = np.where((tok[lo:hi] == v)[:, None], gpos[lo:hi], f32(0))          # (adding 0.f is exact)
            if wide:
                pad = -m.shape[0] % EMBED_WLANES
                m = np.concatenate([m, np.zeros((pad, dim), f32)]).reshape(-1, EMBED_WLANES, dim)
                parts[k] = seq_sum0(seq_sum0(m))
            else:
                parts[k] = seq_sum0(m)
        out[v] = _lane4(parts)
    return out


# =====================================================================================================================
# embed: out row (b, t) = table[clamp(idx[b][t])], rows (b, t) or (t, b);  dtable[v] (+)= sum of the gradient rows whose index clamps to v
# =====================================================================================================================
# (dim, vocab, (batch, steps), time_major, accumulate, pattern).  dim <= 128: embed_bwd_partial_kernel, above: embed_bwd_wide_kernel;
# dim % 4 == 0 and >= 64: the float4 forward, else the scalar one.  Positions: 64 one narrow block, 72 a ragged second one, 888 = 14
# blocks (lanes 2, 3 of the reduce get 3 blocks, lanes 0, 1 get 4), 2064 = 33 blocks (a second trip of the reduce's z0 loop) and
# per = 129 in the wide kernel (a second trip of its i0 loop); 1, 5 under EMBED_WSPLIT (empty position groups), 16 exactly, 17 over.
EMBED_CASES = [
    (1, 1, (1, 1), 0, 0, 'uniform'),
    (1, 35, (1, 5), 1, 1, 'uniform'),
    (10, 35, (1, 16), 0, 1, 'uniform'),
    (10, 35, (1, 17), 1, 0, 'missing'),
    (10, 35, (2, 32), 0, 0, 'uniform'),
    (10, 35, (3, 24), 1, 1, 'out_of_range'),
    (10, 35, (3, 24), 0, 0, 'out_of_range'),
    (10, 300, (37, 24), 1, 0, 'uniform'),
    (10, 35, (86, 24), 0, 1, 'one_token'),
    (10, 63, (86, 24), 1, 0, 'uniform'),
    (64, 35, (3, 24), 1, 0, 'uniform'),                     # the float4 forward with the narrow backward
    (64, 63, (37, 24), 0, 1, 'missing'),
    (100, 35, (37, 24), 1, 1, 'out_of_range'),
    (100, 300, (3, 24), 0, 0, 'uniform'),
    (128, 35, (86, 24), 1, 0, 'out_of_range'),
    (128, 63, (2, 32), 0, 1, 'one_token'),
    (128, 1, (37, 24), 1, 1, 'uniform'),
    (129, 35, (1, 5), 0, 0, 'uniform'),                     # the scalar forward with the wide backward; 11 empty position groups
    (129, 35, (3, 24), 1, 1, 'out_of_range'),
    (130, 35, (1, 16), 1, 0, 'uniform'),
    (130, 63, (37, 24), 0, 1, 'missing'),
    (130, 35, (171, 24), 1, 0, 'uniform'),                  # 4104 x 130 > GRID_CAP: the scalar forward's grid-stride loop twice
    (132, 35, (1, 17), 0, 1, 'uniform'),
    (132, 35, (3, 24), 1, 0, 'out_of_range'),               # the same tokens' treatment at dim 132 as at dim 128 and below
    (132, 35, (86, 24), 0, 0, 'missing'),
    (192, 35, (86, 24), 1, 0, 'one_token'),
    (192, 63, (2, 32), 0, 0, 'uniform'),
    (192, 1, (1, 1), 1, 1, 'uniform'),
    (768, 35, (37, 24), 1, 0, 'out_of_range'),              # the encoder's projection table as Encoder._first_layer_by_lookup uses it
    (768, 63, (3, 24), 0, 1, 'uniform'),
]


def embed_inputs(case):
    dim, vocab, (batch, steps), tm, acc, pattern = case
    rs = _rs('embed', case)
    n = batch * steps
    return dict(dim=dim, vocab=vocab, batch=batch, steps=steps, tm=tm, acc=acc, idx=tokens_for(rs, pattern, vocab, (batch, steps)),
                table=rs.standard_normal((vocab, dim)).astype(f32), g=rs.standard_normal((n, dim)).astype(f32),       # g: rows as `out` has them
                old=rs.standard_normal((vocab, dim)).astype(f32))


def embed_rows(inp, tm=None):
    """position b*steps + t -> its row of out / g"""
    tm = inp['tm'] if tm is None else tm
    pos = np.arange(inp['batch'] * inp['steps'])
    b, t = pos // inp['steps'], pos % inp['steps']
    return t * inp['batch'] + b if tm else pos


def _embed_out(inp, dt, tok, dtable):
    rows = embed_rows(inp)
    out = np.empty((len(rows), inp['dim']), f32)
    out[rows] = inp['table'][tok]
    used = np.zeros(inp['vocab'], bool)
    used[tok] = True
    base = inp['old'] if inp['acc'] else np.zeros_like(inp['old'])
    return dict(x_out=out, dtable=dtable, x_unused_rows=np.ascontiguousarray(base[~used]))


def embed_ref(inp):
    tok = np.clip(inp['idx'].ravel(), 0, inp['vocab'] - 1)
    d = inp['old'].astype(f64) if inp['acc'] else np.zeros(inp['old'].shape, f64)
    np.add.at(d, tok, inp['g'].astype(f64)[embed_rows(inp)])
    return _embed_out(inp, f64, tok, d)


def embed_cpu(inp):
    """torch fp32: index_add_ into the old gradient (or zeros)"""
    tok = np.clip(inp['idx'].ravel(), 0, inp['vocab'] - 1)
    d = _t(inp['old']).clone() if inp['acc'] else torch.zeros(inp['old'].shape)
    d.index_add_(0, _t(tok), _t(inp['g'][embed_rows(inp)]))
    return _embed_out(inp, f32, tok, d.numpy())


def embed_chain(inp, wrong=None):
    tok = np.clip(inp['idx'].ravel(), 0, inp['vocab'] - 1)
    seg_tok = tok
    if wrong == 'gradient index not clamped':                # (int)idx[pos]: outside rows match nothing, 2**32 + 3 lands on row 3
        seg_tok = inp['idx'].ravel().astype(np.int32)
    rows = embed_rows(inp, 1 - inp['tm'] if wrong == 'batch-major rows read as time-major' else None)
    s = segment_sums(inp['g'][rows], seg_tok, inp['vocab'], inp['dim'] > NARROW_MAX, wrong)
    d = inp['old'] + s if inp['acc'] and wrong != 'accumulate overwrites' else s
    out = _embed_out(inp, f32, tok, d)
    used = np.zeros(inp['vocab'], bool)
    used[tok] = True
    out['x_unused_rows'] = np.ascontiguousarray(d[~used])
    return out


# =====================================================================================================================
# tick_rows: x_small = [table | 0; x_0 | 0; 0 | beat_emb] and its adjoint split (dtable, dx0 ADDED, either may be NULL; dbeat written)
# =====================================================================================================================
# (vocab, emb, hidden, rows, stride, null): stride 'dense' = 0, 'hidden' = hidden given explicitly, 'executor' = rows of 3 * hidden floats
# with the beat embedding at column offset hidden (plan_measure.hip: both_ld / 3 * Hd); null: the gradient pointer that is NULL
TICK_ROWS_CASES = [
    (35, 10, 128, 4, 'dense', None), (35, 10, 128, 4, 'executor', 'dtable'), (35, 10, 32, 148, 'hidden', 'dx0'),
    (35, 10, 32, 148, 'executor', None), (1, 1, 4, 1, 'dense', None), (1, 1, 4, 1, 'executor', None), (62, 10, 64, 340, 'executor', None),
    (62, 10, 64, 340, 'dense', 'dtable'),
    (35, 10, 128, 4100, 'executor', None),                  # (36 + 4100) x 138 forward and 360 + 4100 x 128 backward elements: both > GRID_CAP
]
SENTINEL = f32(-12345.5)


def tick_rows_inputs(case):
    vocab, emb, hidden, rows, stride, null = case
    rs = _rs('tick_rows', case)
    ld, off = (3 * hidden, hidden) if stride == 'executor' else (hidden, 0)
    beat = np.full((rows, ld), SENTINEL, f32)
    beat[:, off:off + hidden] = rs.standard_normal((rows, hidden))
    return dict(vocab=vocab, emb=emb, hidden=hidden, rows=rows, ld=ld, off=off, stride_arg=0 if stride == 'dense' else ld, null=null,
                table=rs.standard_normal((vocab, emb)).astype(f32), x0=rs.standard_normal(emb).astype(f32), beat=beat,
                dx=rs.standard_normal((vocab + 1 + rows, emb + hidden)).astype(f32),
                old_table=rs.standard_normal((vocab, emb)).astype(f32), old_x0=rs.standard_normal(emb).astype(f32))


def tick_rows_chain(inp, wrong=None):
    vocab, emb, hidden, rows, off = (inp[k] for k in ('vocab', 'emb', 'hidden', 'rows', 'off'))
    x = np.zeros((vocab + 1 + rows, emb + hidden), f32)
    x[:vocab, :emb], x[vocab, :emb], x[vocab + 1:, emb:] = inp['table'], inp['x0'], inp['beat'][:, off:off + hidden]
    dx = inp['dx']
    dbeat = np.full((rows, inp['ld']), SENTINEL, f32)
    if wrong == 'strided dbeat written densely':
        dbeat.ravel()[off:off + rows * hidden] = dx[vocab + 1:, emb:].ravel()
    else:
        dbeat[:, off:off + hidden] = dx[vocab + 1:, emb:]
    dtable = dx[:vocab, :emb].copy() if wrong == 'accumulate overwrites' else inp['old_table'] + dx[:vocab, :emb]
    out = dict(x_x=x, x_dbeat=dbeat, x_dtable=inp['old_table'].copy() if inp['null'] == 'dtable' else dtable,
               x_dx0=inp['old_x0'].copy() if inp['null'] == 'dx0' else inp['old_x0'] + dx[vocab, :emb])
    return out


def tick_rows_ref(inp):
    """every output is one fp32 value or one fp32 addition: the float64 sum of two fp32 numbers rounds to the same bits"""
    out = tick_rows_chain(inp)
    vocab, emb = inp['vocab'], inp['emb']
    if inp['null'] != 'dtable':
        out['x_dtable'] = (inp['old_table'].astype(f64) + inp['dx'][:vocab, :emb].astype(f64)).astype(f32)
    if inp['null'] != 'dx0':
        out['x_dx0'] = (inp['old_x0'].astype(f64) + inp['dx'][vocab, :emb].astype(f64)).astype(f32)
    return out


def tick_rows_cpu(inp):
    return tick_rows_ref(inp)


# =====================================================================================================================
# tick_gi: gi[(j*beats + beat)*batch + b] = (G[prev] + G[vocab + 1 + beat*batch + b]) + bias and the sums into dG
# =====================================================================================================================
def tick_order(batch, beats, tpb):
    """per gradient row (j, beat, b) of [tpb][beats][batch]: (tick t = tpb*beat + j, measure b, beat row beat*batch + b)"""
    j, beat, b = (a.ravel() for a in np.meshgrid(np.arange(tpb), np.arange(beats), np.arange(batch), indexing='ij'))
    return tpb * beat + j, b, beat * batch + b


def previous_notes(tokens, vocab, batch, beats, tpb, wrong=None):
    """row of [table; x_0] each tick reads: x_0 (row `vocab`) at tick 0, else the clamped previous note"""
    t, b, _ = tick_order(batch, beats, tpb)
    tok = np.clip(tokens, 0, vocab - 1)
    start = 0 if wrong == 'tick 0 takes token 0 instead of x_0' else vocab
    return np.where(t == 0, start, tok[b, np.maximum(t - 1, 0)])


# ((batch, beats, tpb), cols, vocab, pattern, bias).  Positions batch*beats*tpb: 1; 24, 72 (few per group); 888; 2064 (per = 129);
# cols 260: cols4 = 65, a second trip of the forward's lane loop, and a ragged ninth column slice of the segment sum
TICK_GI_CASES = [
    ((1, 1, 1), 4, 1, 'uniform', False), ((1, 1, 1), 96, 35, 'uniform', True), ((1, 4, 6), 384, 35, 'uniform', True),
    ((1, 4, 6), 260, 62, 'out_of_range', False), ((3, 4, 6), 96, 35, 'out_of_range', True), ((3, 4, 6), 384, 62, 'missing', False),
    ((37, 4, 6), 192, 35, 'uniform', True), ((37, 4, 6), 384, 62, 'out_of_range', True), ((5, 2, 12), 96, 35, 'one_token', False),
    ((5, 1, 24), 260, 35, 'uniform', True), ((7, 3, 8), 4, 62, 'uniform', True), ((7, 3, 8), 192, 1, 'uniform', False),
    ((86, 4, 6), 96, 35, 'one_token', True), ((86, 4, 6), 384, 35, 'out_of_range', False),
    ((5500, 1, 2), 384, 35, 'uniform', True),              # 5500 beat rows x 96 float4 > GRID_CAP: tick_gi_bwd_beat_kernel's loop twice
]


def tick_gi_inputs(case):
    (batch, beats, tpb), cols, vocab, pattern, bias = case
    rs = _rs('tick_gi', case)
    rows_b = beats * batch
    return dict(batch=batch, beats=beats, tpb=tpb, cols=cols, vocab=vocab, tokens=tokens_for(rs, pattern, vocab, (batch, beats * tpb)),
                g_small=rs.standard_normal((vocab + 1 + rows_b, cols)).astype(f32),
                bias=rs.standard_normal(cols).astype(f32) if bias else None, dgi=rs.standard_normal((tpb * rows_b, cols)).astype(f32))


def _tick_gi_out(inp, gi, dg_beat, dg_notes, prev):
    vocab = inp['vocab']
    used = np.zeros(vocab + 1, bool)
    used[prev] = True
    return dict(x_gi=gi, x_dg_beat=dg_beat, dg_notes=dg_notes[:vocab], dg_x0=dg_notes[vocab], x_dg_unused_rows=np.ascontiguousarray(dg_notes[~used], f32))


def tick_gi_ref(inp):
    """gi: two fp32 additions in the documented order (no multiply: nothing to contract); the beat rows: the fp32 sum in tick order
    (tick_gi_chain: the header fixes it), the note rows in float64"""
    batch, beats, tpb, vocab = (inp[k] for k in ('batch', 'beats', 'tpb', 'vocab'))
    chain = tick_gi_chain(inp)
    prev = previous_notes(inp['tokens'], vocab, batch, beats, tpb)
    d = np.zeros((vocab + 1, inp['cols']), f64)
    np.add.at(d, prev, inp['dgi'].astype(f64))
    return _tick_gi_out(inp, chain['x_gi'], chain['x_dg_beat'], d, prev)


def tick_gi_cpu(inp):
    batch, beats, tpb, vocab = (inp[k] for k in ('batch', 'beats', 'tpb', 'vocab'))
    prev = previous_notes(inp['tokens'], vocab, batch, beats, tpb)
    _, _, brow = tick_order(batch, beats, tpb)
    g = _t(inp['g_small'])
    gi = g[_t(prev)] + g[_t(vocab + 1 + brow)]
    if inp['bias'] is not None:
        gi = gi + _t(inp['bias'])
    d = torch.zeros(vocab + 1, inp['cols']).index_add_(0, _t(prev), _t(inp['dgi']))
    dgb = torch.zeros(beats * batch, inp['cols']).index_add_(0, _t(brow), _t(inp['dgi']))
    return _tick_gi_out(inp, gi.numpy(), dgb.numpy(), d.numpy(), prev)


def tick_gi_parts(inp, wrong=None):
    """(gi, dG beat rows, dG note rows, prev) in the kernels' order"""
    batch, beats, tpb, vocab, G = (inp[k] for k in ('batch', 'beats', 'tpb', 'vocab', 'g_small'))
    prev = previous_notes(inp['tokens'], vocab, batch, beats, tpb, wrong)
    t, b, brow = tick_order(batch, beats, tpb)
    if wrong == 'beat row index b * beats + beat':
        brow = b * beats + (t // tpb)
    gi = G[prev] + G[vocab + 1 + brow]
    if inp['bias'] is not None:
        gi = gi + inp['bias']
    d3 = inp['dgi'].reshape(tpb, beats * batch, -1)
    dg_beat = seq_sum0(d3[:tpb - 1] if wrong == 'beat rows summed over tpb - 1 ticks' and tpb > 1 else d3)
    if wrong == 'beat row index b * beats + beat':
        dg_beat = dg_beat.reshape(beats, batch, -1).transpose(1, 0, 2).reshape(beats * batch, -1)
    return gi.astype(f32), dg_beat, segment_sums(inp['dgi'], prev, vocab + 1, True, wrong), prev


def tick_gi_chain(inp, wrong=None):
    gi, dg_beat, dg_notes, _ = tick_gi_parts(inp, wrong)
    right = previous_notes(inp['tokens'], inp['vocab'], inp['batch'], inp['beats'], inp['tpb'])
    return _tick_gi_out(inp, gi, dg_beat, dg_notes, right)


# =====================================================================================================================
# tick_projection: gi = W_ih0 [emb(prev) | beat_emb] + b_ih0 per tick, x_0 at tick 0 (ops.tick_input_projection and the model's fallback)
# =====================================================================================================================
# (hidden, batch, vocab, preset): 4 beats x 6 ticks, embeddings of 10; preset: the leaf parameters own a .grad that is added to.
# vocab 62 at batch 85: the segment sum's LDS guard passes by one position, 63 * 1024 + 128 * 8 = 65536
PROJ_BEATS, PROJ_TPB, PROJ_EMB = 4, 6, 10
TICK_PROJECTION_CASES = [(h, b, 35, bool((i + k) % 2)) for i, h in enumerate((32, 64, 128)) for k, b in enumerate((1, 3, 37))] + \
                        [(128, 85, 62, False), (128, 37, 35, True)]


def tick_projection_inputs(case):
    hidden, batch, vocab, preset = case
    rs = _rs('tick_projection', case)
    emb, rows_b, cols = PROJ_EMB, PROJ_BEATS * batch, 3 * hidden
    sd = 1.0 / np.sqrt(emb + hidden)
    inp = dict(hidden=hidden, batch=batch, beats=PROJ_BEATS, tpb=PROJ_TPB, vocab=vocab, emb=emb, cols=cols, preset=preset,
               tokens=tokens_for(rs, 'out_of_range' if batch == 3 else 'uniform', vocab, (batch, PROJ_BEATS * PROJ_TPB)),
               table=rs.standard_normal((vocab, emb)).astype(f32), x0=rs.uniform(-1, 1, emb).astype(f32),
               beat_emb=rs.standard_normal((rows_b, hidden)).astype(f32), w_ih=(sd * rs.standard_normal((cols, emb + hidden))).astype(f32),
               b_ih=rs.uniform(-0.1, 0.1, cols).astype(f32), dgi=rs.standard_normal((PROJ_TPB * rows_b, cols)).astype(f32))
    for k in ('table', 'x0', 'w_ih', 'b_ih'):
        inp['old_' + k] = rs.standard_normal(inp[k].shape).astype(f32) if preset else None
    return inp


def _proj_finish(inp, dt, gi, d):
    for k in ('table', 'x0', 'w_ih', 'b_ih'):
        if inp['preset']:
            d[k] = inp['old_' + k].astype(dt) + d[k]
    return dict(gi=gi, d_table=d['table'], d_x0=d['x0'], d_beat=d['beat'], d_w=d['w_ih'], d_b=d['b_ih'])


def tick_projection_ref(inp):
    """the reference formulation in float64 numpy, its backward written out"""
    batch, beats, tpb, vocab, emb = (inp[k] for k in ('batch', 'beats', 'tpb', 'vocab', 'emb'))
    prev = previous_notes(inp['tokens'], vocab, batch, beats, tpb)
    _, _, brow = tick_order(batch, beats, tpb)
    e = np.concatenate([inp['table'], inp['x0'][None]]).astype(f64)
    x = np.concatenate([e[prev], inp['beat_emb'].astype(f64)[brow]], 1)
    w, dgi = inp['w_ih'].astype(f64), inp['dgi'].astype(f64)
    gi = x @ w.T + inp['b_ih'].astype(f64)
    dx = dgi @ w
    de, dbeat = np.zeros_like(e), np.zeros(inp['beat_emb'].shape, f64)
    np.add.at(de, prev, dx[:, :emb])
    np.add.at(dbeat, brow, dx[:, emb:])
    return _proj_finish(inp, f64, gi, dict(table=de[:vocab], x0=de[vocab], beat=dbeat, w_ih=dgi.T @ x, b_ih=dgi.sum(0)))


def tick_projection_torch(inp, dt):
    """the reference formulation in torch (dt), gradients by autograd; .grad pre-set where the case says so"""
    batch, beats, tpb, vocab = (inp[k] for k in ('batch', 'beats', 'tpb', 'vocab'))
    prev = _t(previous_notes(inp['tokens'], vocab, batch, beats, tpb))
    brow = _t(tick_order(batch, beats, tpb)[2])
    p = {k: _t(inp[k]).to(dt).requires_grad_(True) for k in ('table', 'x0', 'beat_emb', 'w_ih', 'b_ih')}
    for k in ('table', 'x0', 'w_ih', 'b_ih'):
        if inp['preset']:
            p[k].grad = _t(inp['old_' + k]).to(dt).clone()
    x = torch.cat([torch.cat([p['table'], p['x0'][None]])[prev], p['beat_emb'][brow]], 1)
    gi = F.linear(x, p['w_ih'], p['b_ih'])
    gi.backward(_t(inp['dgi']).to(dt))
    return dict(gi=gi.detach().numpy(), d_table=p['table'].grad.numpy(), d_x0=p['x0'].grad.numpy(), d_beat=p['beat_emb'].grad.numpy(),
                d_w=p['w_ih'].grad.numpy(), d_b=p['b_ih'].grad.numpy())


def tick_projection_cpu(inp):
    return tick_projection_torch(inp, torch.float32)


def tick_projection_chain(inp, wrong=None):
    """the re-associated form in fp32 numpy: X, G = X W^T, the gather, the segment sums into dG, dX = dG W, dW = dG^T X,
    db = column sums of dG's note rows"""
    vocab, emb, hidden, rows_b = inp['vocab'], inp['emb'], inp['hidden'], inp['beats'] * inp['batch']
    x = np.zeros((vocab + 1 + rows_b, emb + hidden), f32)
    x[:vocab, :emb], x[vocab, :emb], x[vocab + 1:, emb:] = inp['table'], inp['x0'], inp['beat_emb']
    gi, dg_beat, dg_notes, _ = tick_gi_parts(dict(inp, g_small=x @ inp['w_ih'].T, bias=inp['b_ih']), wrong)
    dg = np.concatenate([dg_notes, dg_beat])
    dx = dg @ inp['w_ih']
    return _proj_finish(inp, f32, gi, dict(table=dx[:vocab, :emb], x0=dx[vocab, :emb], beat=dx[vocab + 1:, emb:], w_ih=dg.T @ x,
                                           b_ih=seq_sum0(dg_notes)))


# =====================================================================================================================
# small ops.  concat_cols / split_cols / scale_mask / broadcast_rows: every output is a copy, one fp32 product or one fp32 sum
# =====================================================================================================================
# ('concat', rows, (ca, cb)) | ('split', rows, (ca, cb), accumulate_b) | ('scale', count, accumulate, mask, alpha) | ('bcast', rows, cols)
BIG_ROWS = 3800                                             # x (10 + 128) = 524 400 elements > GRID_CAP
COPY_CASES = ([('concat', r, w) for r in (1, 7) for w in ((1, 1), (10, 128), (100, 38))] + [('concat', BIG_ROWS, (10, 128))] +
              [('split', r, w, a) for r in (1, 7) for w in ((1, 1), (10, 128), (100, 38)) for a in (0, 1)] +
              [('split', BIG_ROWS, (10, 128), 1)] +
              # alpha: 2 = 1 / (1 - 0.5), the model's dropout scale, wherever y is added to (2 x is exact, so the result does not depend on
              # whether the compiler contracts the product into the sum); 1 / 0.7 where the product is stored as it is
              [('scale', n, a, m, 2.0) for n in (1, 7, GRID_CAP + 13) for a in (0, 1) for m in (False, True)] +
              [('scale', n, 0, m, 1.0 / 0.7) for n in (7, 1000) for m in (False, True)] +
              [('bcast', 1, 10), ('bcast', 7, 128), ('bcast', 7, 1), ('bcast', 4100, 128)])


def copy_inputs(case):
    rs = _rs('copy', case)
    kind = case[0]
    if kind in ('concat', 'split'):
        rows, (ca, cb) = case[1], case[2]
        return dict(kind=kind, rows=rows, ca=ca, cb=cb, acc=case[3] if kind == 'split' else 0, a=rs.standard_normal((rows, ca)).astype(f32),
                    b=rs.standard_normal((rows, cb)).astype(f32), g=rs.standard_normal((rows, ca + cb)).astype(f32))
    if kind == 'scale':
        _, n, acc, mask, alpha = case
        return dict(kind=kind, n=n, acc=acc, alpha=f32(alpha), x=rs.standard_normal(n).astype(f32), y=rs.standard_normal(n).astype(f32),
                    mask=(rs.random_sample(n) < 0.5).astype(np.uint8) if mask else None)
    return dict(kind=kind, rows=case[1], cols=case[2], v=rs.standard_normal(case[2]).astype(f32))


def copy_chain(inp, wrong=None):
    kind = inp['kind']
    if kind == 'concat':
        return dict(x_out=np.concatenate([inp['a'], inp['b']], 1))
    if kind == 'split':
        ca, g = inp['ca'], inp['g']
        return dict(x_da=np.ascontiguousarray(g[:, :ca]),
                    x_db=inp['b'] + g[:, ca:] if inp['acc'] and wrong != 'accumulate overwrites' else np.ascontiguousarray(g[:, ca:]))
    if kind == 'scale':
        v = inp['alpha'] * inp['x']
        if inp['mask'] is not None and wrong != 'mask ignored':
            v = v * inp['mask'].astype(f32)
        return dict(x_y=(inp['y'] + v if inp['acc'] else v).astype(f32))
    return dict(x_y=np.ascontiguousarray(np.broadcast_to(inp['v'], (inp['rows'], inp['cols']))))


def copy_ref(inp):
    """the float64 product of two fp32 numbers is exact, and a float64 sum of two fp32 numbers rounds to fp32 as their fp32 sum does"""
    out = copy_chain(inp)
    if inp['kind'] == 'split' and inp['acc']:
        out['x_db'] = (inp['b'].astype(f64) + inp['g'][:, inp['ca']:].astype(f64)).astype(f32)
    if inp['kind'] == 'scale':
        v = (f64(inp['alpha']) * inp['x'].astype(f64)).astype(f32).astype(f64)
        if inp['mask'] is not None:
            v = v * inp['mask']
        out['x_y'] = (inp['y'].astype(f64) + v if inp['acc'] else v).astype(f32)
    return out


def copy_cpu(inp):
    return copy_ref(inp)


# ---- GRU gates: r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h;  dgi, dgh, dh_prev from dh
# (hidden, batch, h_prev given, amplitude of the pre-activations)
GRU_GATES_CASES = [(h, b, hp, 1.0) for h in (32, 64, 128) for b in (1, 37) for hp in (False, True)] + \
                  [(64, 37, True, 30.0),                     # pre-activations up to +-30 (their sums to +-60): saturated gates
                   (128, 4100, True, 1.0)]                   # 524 800 elements > GRID_CAP


def gru_gates_inputs(case):
    hidden, batch, hp, amp = case
    rs = _rs('gru_gates', case)
    draw = (lambda s: rs.uniform(-amp, amp, s)) if amp > 1.0 else (lambda s: rs.standard_normal(s))
    return dict(hidden=hidden, batch=batch, gi=draw((batch, 3 * hidden)).astype(f32), gh=draw((batch, 3 * hidden)).astype(f32),
                h_prev=rs.standard_normal((batch, hidden)).astype(f32) if hp else None, dh=rs.standard_normal((batch, hidden)).astype(f32))


def gru_gates_torch(inp, dt):
    gi, gh = (_t(inp[k]).to(dt).requires_grad_(True) for k in ('gi', 'gh'))
    hp = None if inp['h_prev'] is None else _t(inp['h_prev']).to(dt).requires_grad_(True)
    hid = inp['hidden']
    r = torch.sigmoid(gi[:, :hid] + gh[:, :hid])
    z = torch.sigmoid(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
    n = torch.tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
    h = (1 - z) * n + (z * hp if hp is not None else 0)
    h.backward(_t(inp['dh']).to(dt))
    out = dict(h=h.detach().numpy(), dgi=gi.grad.numpy(), dgh=gh.grad.numpy())
    if hp is not None:
        out['dh_prev'] = hp.grad.numpy()
    return out


def gru_gates_ref(inp):
    return gru_gates_torch(inp, torch.float64)


def gru_gates_cpu(inp):
    """the same formulas in torch fp32, gradients by autograd"""
    return gru_gates_torch(inp, torch.float32)


def gru_gates_chain(inp, wrong=None):
    """gru_gates_fwd_kernel / gru_gates_bwd_kernel in fp32 numpy"""
    hid, one = inp['hidden'], f32(1)
    gi, gh, g = inp['gi'], inp['gh'], inp['dh']
    hp = np.zeros_like(g) if inp['h_prev'] is None else inp['h_prev']
    sig = lambda x: one / (one + np.exp(-x))
    r, z = sig(gi[:, :hid] + gh[:, :hid]), sig(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
    ghn = gh[:, 2 * hid:]
    n = np.tanh(gi[:, 2 * hid:] + r * ghn)
    dpn = g * (one - z) * (one - n * n)
    dpz = g * (hp - n) * z * (one - z)
    dpr = dpn * ghn * r * (one - r)
    dgh_n = dpn if wrong == 'dgh_n without the reset gate' else dpn * r
    out = dict(h=(one - z) * n + z * hp, dgi=np.concatenate([dpr, dpz, dpn], 1), dgh=np.concatenate([dpr, dpz, dgh_n], 1))
    if inp['h_prev'] is not None:
        out['dh_prev'] = g * z
    return out


# =====================================================================================================================
# measure attributes: [rhythmic complexity, pitch range / 26, note density, contour / 26] per measure
# =====================================================================================================================
ATTR_CASES = [(steps, batch) for steps in (1, 7, 8, 9, 24, 25) for batch in (1, 63, 64, 65, 130)]
ATTR_KINDS = ('no_note', 'one_note', 'first_highest', 'outside', 'plain')


def attr_tables():
    from arvae_amd import synthetic as syn
    return syn.measure_tables()


def attr_kind(case, row):
    return ATTR_KINDS[(row + ATTR_CASES.index(case)) % len(ATTR_KINDS)]


def attr_inputs(case):
    """every measure is built for its kind (attr_kind): no note at all; exactly one; the first note the highest of several; tokens
    outside the vocabulary among the rest; or plain random (slurs 60 %)"""
    from oracle.attributes import RHY_COEFFS
    steps, batch = case
    rs = _rs('attr', case)
    midi, is_note, is_dens = attr_tables()
    vocab = len(midi)
    notes, others = np.flatnonzero(is_note), np.flatnonzero(is_note == 0)
    score = np.where(rs.random_sample((batch, steps)) < 0.6, 0, rs.randint(1, vocab, (batch, steps))).astype(np.int64)
    for r in range(batch):
        kind = attr_kind(case, r)
        if kind == 'no_note':
            score[r] = rs.choice(others, steps)
        elif kind == 'one_note':
            score[r] = rs.choice(others, steps)
            score[r, rs.randint(steps)] = rs.choice(notes)
        elif kind == 'first_highest' and steps >= 2:
            by_pitch = notes[np.argsort(midi[notes], kind='stable')]
            lower = notes[midi[notes] < midi[by_pitch[-1]]]
            score[r] = np.where(rs.random_sample(steps) < 0.5, rs.choice(lower, steps), rs.choice(others, steps))
            score[r, 0], score[r, steps - 1] = by_pitch[-1], by_pitch[0]
        elif kind == 'outside':
            score[r, ::3] = rs.choice([-1, -7, vocab, vocab + 5, 2 ** 32 + 3], len(score[r, ::3]))
    w = np.resize(RHY_COEFFS, steps).astype(f32)
    return dict(steps=steps, batch=batch, vocab=vocab, score=score, tables=(midi, is_note, is_dens), w=w, norm=float(w.sum(dtype=f32)))


def attr_coverage():
    """what the table contains, counted from the inputs themselves -> dict kind -> number of measures"""
    seen = dict(no_note=0, one_note=0, first_highest=0, outside=0)
    for case in ATTR_CASES:
        inp = attr_inputs(case)
        midi, is_note, _ = inp['tables']
        for row in inp['score']:
            out = (row < 0) | (row >= inp['vocab'])
            m = midi[np.clip(row, 0, inp['vocab'] - 1)][is_note[np.clip(row, 0, inp['vocab'] - 1)] != 0]
            seen['outside'] += bool(out.any())
            seen['no_note'] += m.size == 0
            seen['one_note'] += m.size == 1
            seen['first_highest'] += m.size >= 2 and m[0] == m.max() and m[0] > m[1:].max()
    return seen


def _attr_out(a, rhythm):
    return dict(rhythm=rhythm, x_range=np.ascontiguousarray(a[:, 1]), x_density=np.ascontiguousarray(a[:, 2]), x_contour=np.ascontiguousarray(a[:, 3]))


def _attr_oracle(inp):
    from oracle.attributes import attribute_labels
    score = np.clip(inp['score'], 0, inp['vocab'] - 1)       # the kernel documents the clamp
    return score, attribute_labels(score, *inp['tables'], rhythm_weights=inp['w'])


def attr_ref(inp):
    """oracle.attributes.attribute_labels; the rhythm sum again in float64, over the kernel's fp32 norm"""
    score, a = _attr_oracle(inp)
    onset = inp['tables'][1][score] != 0
    return _attr_out(a, (inp['w'].astype(f64)[None] * onset).sum(1) / float(f32(inp['norm'])))


def attr_cpu(inp):
    _, a = _attr_oracle(inp)
    return _attr_out(a, a[:, 0])


def attr_chain(inp, wrong=None):
    """measure_attributes_rows in numpy: one walk along the measure"""
    midi, is_note, is_dens = inp['tables']
    score = np.clip(inp['score'], 0, inp['vocab'] - 1)
    out = np.zeros((inp['batch'], 4), f32)
    for r, row in enumerate(score):
        rhy, m = f32(0), []
        for t, v in enumerate(row):
            if is_note[v]:
                rhy = f32(rhy + inp['w'][t])
                m.append(int(midi[v]))
        out[r, 0] = rhy / f32(inp['norm'])
        out[r, 2] = f32(int(is_dens[row].sum())) / f32(inp['steps'])
        if len(m) >= 2:
            out[r, 1] = f32(max(m) - min(m)) / f32(26)
            out[r, 3] = f32(m[0] - m[-1] if wrong == 'contour taken as first - last' else m[-1] - m[0]) / f32(26)
        elif len(m) == 1 and wrong == 'one-note measure reports a range':     # lo left at its initial 0
            out[r, 1] = f32(m[0]) / f32(26)
    return _attr_out(out, out[:, 0])


# =====================================================================================================================
FAMILIES = {
    'embed': (EMBED_CASES, embed_inputs, embed_ref, embed_cpu, embed_chain),
    'tick_rows': (TICK_ROWS_CASES, tick_rows_inputs, tick_rows_ref, tick_rows_cpu, tick_rows_chain),
    'tick_gi': (TICK_GI_CASES, tick_gi_inputs, tick_gi_ref, tick_gi_cpu, tick_gi_chain),
    'tick_projection': (TICK_PROJECTION_CASES, tick_projection_inputs, tick_projection_ref, tick_projection_cpu, tick_projection_chain),
    'copy': (COPY_CASES, copy_inputs, copy_ref, copy_cpu, copy_chain),
    'gru_gates': (GRU_GATES_CASES, gru_gates_inputs, gru_gates_ref, gru_gates_cpu, gru_gates_chain),
    'attr': (ATTR_CASES, attr_inputs, attr_ref, attr_cpu, attr_chain),
}
# planted defect -> [(family, a case of its table that must fail the bar with it)]
WRONG_KERNELS = {
    'gradient index not clamped': [('embed', (10, 35, (3, 24), 1, 1, 'out_of_range')), ('embed', (128, 35, (86, 24), 1, 0, 'out_of_range'))],
    'batch-major rows read as time-major': [('embed', (10, 35, (2, 32), 0, 0, 'uniform')), ('embed', (130, 63, (37, 24), 0, 1, 'missing'))],
    'last partial block dropped': [('embed', (10, 35, (3, 24), 0, 0, 'out_of_range'))],
    'last position group dropped': [('embed', (132, 35, (3, 24), 1, 0, 'out_of_range')), ('tick_gi', ((3, 4, 6), 96, 35, 'out_of_range', True))],
    'accumulate overwrites': [('embed', (10, 35, (1, 16), 0, 1, 'uniform')), ('tick_rows', (35, 10, 128, 4, 'dense', None)),
                              ('copy', ('split', 7, (10, 128), 1))],
    'tick 0 takes token 0 instead of x_0': [('tick_gi', ((3, 4, 6), 96, 35, 'out_of_range', True)), ('tick_projection', (64, 3, 35, False))],
    'beat rows summed over tpb - 1 ticks': [('tick_gi', ((7, 3, 8), 4, 62, 'uniform', True)), ('tick_projection', (32, 1, 35, False))],
    'beat row index b * beats + beat': [('tick_gi', ((37, 4, 6), 192, 35, 'uniform', True)), ('tick_projection', (128, 37, 35, True))],
    'strided dbeat written densely': [('tick_rows', (35, 10, 32, 148, 'executor', None))],
    'mask ignored': [('copy', ('scale', 7, 1, True, 2.0))],
    'dgh_n without the reset gate': [('gru_gates', (32, 1, False, 1.0))],
    'contour taken as first - last': [('attr', (24, 64))],
    'one-note measure reports a range': [('attr', (8, 63))],
}

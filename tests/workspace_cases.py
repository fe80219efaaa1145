"""The table of the workspace-contract test (test_workspace_contract_gpu.py): family -> cases, each one driver call at the smallest
shapes at which its scratch logic branches.  No test in here; test_workspace_cases.py holds the table to its promises on the CPU.

The contract: an entry point that takes caller-allocated scratch gets EXACTLY what its `*_ws_floats` /
`*_ws_bytes` function reported, with arbitrary prior contents, and stores nothing outside any caller buffer.  The GPU test runs
every case three ways -- the plain allocator, guarded_alloc with the NaN fill, guarded_alloc with the big-finite fill -- and
compares every tensor a case returns bit for bit.

A case is  Case(family, name, sizes, run):
  sizes(lib) -> the scratch sizes the library reports for the case's calls (host code: no GPU needed)
  run(dev)   -> {name: tensor} of every returned tensor and every caller-provided accumulator, inputs made from the case
                modules' own generators (split_cases, single_channel_cases, loss_cases, sequence_cases, gru_cases, resnet_ref,
                arvae_amd.synthetic): seeded, so three runs see the same bytes

EXCEPTIONS lists the buffers a wrapper legitimately hands back partly unwritten: one row per buffer at one call site, with the
code line that makes it so.  Never a family, never a wildcard."""
import ctypes
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import gru_cases
import loss_cases as lc
import resnet_ref
import sequence_cases as sq
import single_channel_cases as sc
import split_cases as sp
from arvae_amd import synthetic as syn

Case = namedtuple('Case', 'family name sizes run')

# (case name, key of the returned tensor, call site of its allocation, why it is partly unwritten)
EXCEPTIONS = []

FAMILIES = ('links-conv32', 'links-conv64', 'links-single-channel', 'channel_sum', 'wide_dense', 'dense', 'loss', 'sequence',
            'tick_decoders', 'classifier', 'ksg', 'executors')
EXECUTOR_FAMILY = 'executors'


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _to(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


# =====================================================================================================================
# links: ops.link_down / link_up / link_wgrad
# =====================================================================================================================
def _link(hh, hw, chi, lh, lw, clo, k, s, p):
    from arvae_amd import ops
    return ops.Link(hh, hw, chi, lh, lw, clo, k, k, s, p)


def _link_sizes(link, n, wants):
    def sizes(lib):
        d = link.desc(n)
        out = []
        if 'down' in wants or 'up' in wants:
            out.append(lib.arvae_link_ws_floats(ctypes.byref(d)))
        if any(w.startswith('wgrad') for w in wants):
            out.append(lib.arvae_link_wgrad_ws_floats(ctypes.byref(d)))
        return out
    return sizes


def _link_tensors(link, n, key):
    """channels-last fp32 tensors of a link: hi, lo, weights [clo][chi][k][k] (x 0.2), the two biases"""
    seed = _seed('link', key)
    return dict(hi=syn.normal_noise((n, link.hh, link.hw, link.chi), seed), lo=syn.normal_noise((n, link.lh, link.lw, link.clo), seed + 1),
                w=0.2 * syn.normal_noise((link.clo, link.chi, link.kh, link.kw), seed + 2), b_lo=syn.normal_noise((link.clo,), seed + 3),
                b_hi=syn.normal_noise((link.chi,), seed + 4))


def _fold_tensors(t, side, act, masked, key):
    """the saved output y (and keep-mask) of a gradient operand (g, y, mask, act) on `side`, as test_split_kernels_float64 makes them"""
    seed = _seed('fold', key)
    y = syn.normal_noise(t[side].shape, seed)
    if act == 1:
        y = np.maximum(y, 0)                                     # a saved ReLU output
    if masked:
        m = syn.dropout_masks([t[side].shape], seed + 1)[0]
        y = (y * m * 2.0).astype(np.float32)                     # ... of a layer with dropout: kept values times two
        t[f'm_{side}'] = m
    t[f'y_{side}'] = y
    return t


def _run_link(dev, link, n, t, wants, fold=None, bias=True):
    """wants: 'down', 'up', 'wgrad0' / 'wgrad1' / 'wgrad2' (link_wgrad with that bias_side) -> every output and accumulator"""
    from arvae_amd import ops
    d = {k: _to(v, dev) for k, v in t.items() if isinstance(v, np.ndarray)}

    def op(side):
        if fold is not None and fold[0] == side:
            return ops._operand(d[side], d[f'y_{side}'], d.get(f'm_{side}'), fold[1])
        return ops._operand(d[side])
    out = {}
    if 'down' in wants:
        out['down'] = ops.link_down(link, n, op('hi'), d['w'], d['b_lo'] if bias else None, ops.ACT_NONE, d.get('m_out'))
    if 'up' in wants:
        out['up'] = ops.link_up(link, n, op('lo'), d['w'], d['b_hi'] if bias else None, ops.ACT_NONE, d.get('m_out'))
    for side in (0, 1, 2):
        if f'wgrad{side}' not in wants:
            continue
        dw = torch.zeros_like(d['w'])
        db = None if side == 0 else torch.zeros(link.clo if side == 1 else link.chi, device=dev)
        ops.link_wgrad(link, n, op('lo'), op('hi'), dw, db, side)
        out[f'dw{side}'] = dw
        if db is not None:
            out[f'db{side}'] = db
    out['_keep'] = d                                             # the operands hold raw pointers: alive until the caller has synchronised
    return out


def _link_case(family, name, link, n, wants, fold=None):
    def run(dev):
        t = _link_tensors(link, n, name)
        if fold is not None:
            _fold_tensors(t, fold[0], fold[1], fold[2], name)
        return _run_link(dev, link, n, t, wants, fold)
    return Case(family, name, _link_sizes(link, n, wants), run)


def _conv32_cases():
    """32 <-> 32 channels, k4 s2 p1 (conv32.hip): lo 16, 8 and 4; one image and five; the weight gradient with every bias_side"""
    out = []
    for size in (16, 8, 4):
        link = _link(2 * size, 2 * size, 32, size, size, 32, 4, 2, 1)
        for n in (1, 5):
            out.append(_link_case('links-conv32', f'conv32-lo{size}-n{n}', link, n, ('down', 'up', 'wgrad0', 'wgrad1', 'wgrad2')))
    return out


def _split_link(name):
    hi, chi, lo, clo, pad, k = sp.link_geometry(name)
    return _link(hi, hi, chi, lo, lo, clo, k, 1, pad)


def _conv64_cases():
    fam, out = 'links-conv64', []
    for name in sp.CONV_LINKS:                                   # every forward link at n = 3
        out.append(_link_case(fam, f'{name}-n3', _split_link(name), 3, ('down', 'up')))
    for act in (1, 2):                                           # the folded operands on the 64 <-> 64 layer: the operand-AMAX pass uses scratch
        for masked in (False, True):
            for side, wants in (('lo', ('up', 'wgrad1')), ('hi', ('down', 'wgrad2'))):
                tag = f'c64_25-n3-{side}_{"relu" if act == 1 else "selu"}{"_mask" if masked else ""}'
                out.append(_link_case(fam, tag, _split_link('c64_25'), 3, wants, fold=(side, act, masked)))
    largest = {}
    for name, n in sp.WGRAD_CASES:
        largest[name] = max(largest.get(name, 0), n)
    for name, n_max in largest.items():                          # the weight gradients at one image and at their largest batch
        for n in (1, n_max):
            out.append(_link_case(fam, f'{name}-wgrad-n{n}', _split_link(name), n, ('wgrad1', 'wgrad2')))
    return out


GENERIC_WGRAD = sc.geom(32, 32, 64)                              # lw = 29: outside conv_c1w_fits -> link_gemm_kernel with z-split slabs


def _single_channel_selection():
    """one case per kernel of single_channel_cases, every `-generic` neighbour, and the generic weight gradient at n = 1 (pix = 841:
    max_split = ceil(841 / BK) clamps the z-split) and n = 3 (pix = 2523, no multiple of the chunk)"""
    seen, picked = set(), []
    for c in sc.CASES:
        if c.kernel == sc.GENERIC or c.kernel not in seen:
            seen.add(c.kernel)
            picked.append(c)
    generic = next(c for c in sc.OUTSIDE_CASES if c.route == 'wgrad')
    assert generic.geom == GENERIC_WGRAD
    picked += [generic._replace(n=1), generic._replace(n=3)]
    return picked


def _single_channel_case(case):
    g = case.geom
    link = _link(g.hh, g.hw, 1, g.lh, g.lw, g.clo, g.k, g.s, g.p)
    n = sc.batch(case)
    wants = {'down': ('down',), 'up': ('up',), 'wgrad': ('wgrad1', 'wgrad2')}[case.route]
    fold = None if case.fold is None else (case.fold[0], case.fold[1])

    def run(dev):
        return _run_link(dev, link, n, sc.inputs(case), wants, fold, case.bias)
    return Case('links-single-channel', sc.case_id(case), _link_sizes(link, n, wants), run)


# =====================================================================================================================
# ops.channel_sum, ops.wide_dense, ops.dense
# =====================================================================================================================
CHANNEL_SUM_ROWS = (1, 15, 17, 16385)                            # 16385: above the 1024-block clamp, rpb = 17, the last block short
CHANNEL_SUM_CHANNELS = (8, 64, 10)                               # 8, 64: channel_sum4_kernel (float4); 10: channel_sum_kernel (scalar)


def _channel_sum_case(rows, channels, folded=False):
    name = f'channel_sum-r{rows}-c{channels}' + ('-folded' if folded else '')

    def run(dev):
        from arvae_amd import ops
        seed = _seed(name)
        x = _to(syn.normal_noise((rows, channels), seed), dev)
        keep = [x]
        if folded:                                               # (g, y, mask, ReLU): the scalar kernel's Operand path
            y = _to(np.maximum(syn.normal_noise((rows, channels), seed + 1), 0), dev)
            m = _to(syn.dropout_masks([(rows, channels)], seed + 2)[0], dev)
            op = ops._operand(x, y, m, ops.ACT_RELU)
            keep += [y, m]
        else:
            op = ops._operand(x)
        out = _to(syn.normal_noise((channels,), seed + 3), dev)  # accumulates: a non-zero start
        ops.channel_sum(op, rows, channels, (0, 0), out)
        return dict(out=out, _keep=keep)
    return Case('channel_sum', name, lambda lib: [lib.arvae_channel_sum_ws_floats(rows, channels)], run)


def _dense_tensors(rows, fin, fout):
    seed = _seed('dense', rows, fin, fout)
    return (syn.normal_noise((rows, fin), seed), (syn.normal_noise((fout, fin), seed + 1) / np.sqrt(fin)).astype(np.float32),
            syn.normal_noise((fout,), seed + 2), syn.normal_noise((rows, fout), seed + 3))


def _wide_dense_case(case, mode):
    rows, fin, fout, in_perm, out_perm = case
    name = f'wide_dense-{rows}x{fin}to{fout}-mode{mode}'

    def link():
        from arvae_amd import ops
        return ops.Link.dense(fin, fout, in_perm=in_perm, out_perm=out_perm)

    def run(dev):
        from arvae_amd import ops
        x, w, b, gy = (_to(a, dev) for a in _dense_tensors(rows, fin, fout))
        if mode == 0:                                            # (the split reduction's consumer adds the bias: one pass only has one)
            return dict(y=ops.wide_dense(link(), rows, 0, w, x=x, bias=b if fin < fout else None))
        if mode == 1:
            return dict(dx=ops.wide_dense(link(), rows, 1, w, g=gy))
        dw, db = torch.zeros_like(w), torch.zeros_like(b)
        ops.wide_dense(link(), rows, 2, w, x=x, g=gy, dw=dw, dbias=db)
        return dict(dw=dw, db=db)
    return Case('wide_dense', name, lambda lib: [lib.arvae_wide_dense_ws_floats(ctypes.byref(link().desc(rows)))], run)


DENSE_LONG = [c for c in sp.DENSE_LONG if c[:3] in ((2050, 138, 384), (2048, 256, 130))]      # rows-GEMM slices
DENSE_SMALL = sp.DENSE_SMALL[1]                                  # (33, 256, 10): inside a backward pass, the deferred flush


def _dense_case(case, preset_grads):
    """ops.dense forward + backward.  preset_grads: the parameters own .grad buffers, so the weight gradient is queued and leaves
    with the backward pass's closing dense_wgrad_batch launch (ops._defer_dense_wgrad)"""
    rows, fin, fout, in_perm, out_perm = case
    name = f'dense-{rows}x{fin}to{fout}' + ('-deferred' if preset_grads else '')

    def sizes(lib):
        from arvae_amd import ops
        d = ops.Link.dense(fin, fout).desc(rows)
        return [lib.arvae_link_ws_floats(ctypes.byref(d)), lib.arvae_link_wgrad_ws_floats(ctypes.byref(d))]

    def run(dev):
        from arvae_amd import ops
        x, w, b, gy = _dense_tensors(rows, fin, fout)
        xd, wd, bd = (_to(a, dev, True) for a in (x, w, b))
        if preset_grads:
            wd.grad, bd.grad = torch.zeros_like(wd), torch.zeros_like(bd)
        yd = ops.dense(xd, wd, bd, ops.Link.dense(fin, fout, in_perm=in_perm, out_perm=out_perm), 0)
        yd.backward(_to(gy, dev))
        assert not ops._WGRAD_QUEUE
        return dict(y=yd.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)
    return Case('dense', name, sizes, run)


# =====================================================================================================================
# loss side
# =====================================================================================================================
def _first(cases, pred):
    return next(c for c in cases if pred(c))


REG_PICKS = [_first(lc.REG_CASES, lambda c, s=s: c[0] == s) for s in ('n1', 'n9', 'rows5', 'n2049')]      # smallest; ragged; row block; past a chunk
IMAGE_PICKS = [_first(lc.IMAGE_CASES, lambda c, d=d, s=s: c[0] == d and c[1] == s and c[2] == 'mixed')
               for d in ('bernoulli', 'gaussian') for s in ((1, 1), (3, 1, 5, 7), (2, 4099))]
TOKEN_PICKS = [_first(lc.TOKEN_CASES, lambda c, s=s: c[0] == s and c[1] == 'normal') for s in ((1, 1), (65, 49), (200, 130))]


def _reg_case(case):
    rows, _row0, _cols, _ldz, _ldl, dims = lc.REG_SHAPES[case[0]]

    def run(dev):
        from arvae_amd import ops
        inp = lc.reg_inputs(case)
        rows, row0 = inp['rows'], inp['row0']
        z_all, lab_all = _to(inp['z'], dev), _to(inp['lab'], dev)
        z = z_all[row0:row0 + rows].clone().requires_grad_(True)
        square = rows == inp['cols']
        loss = ops.reg_loss(z, lab_all[row0:row0 + rows].clone(), inp['dims'], lc.REG_GAMMA, inp['delta'],
                            None if square else z_all, None if square else lab_all)
        (lc.REG_UPSTREAM * loss).backward()
        return dict(loss=loss.detach(), dz=z.grad)
    return Case('loss', 'reg-' + lc.case_id(case), lambda lib: [lib.arvae_reg_loss_ws_floats(rows, len(dims))], run)


def _image_case(case):
    def run(dev):
        from arvae_amd import ops
        inp = lc.image_inputs(case)
        logits, x = _to(inp['logits'], dev, True), _to(inp['x'], dev)
        loss, acc = ops.image_recon(logits, x, inp['dist'])
        loss.backward()
        return dict(loss=loss.detach(), acc=acc, dlogits=logits.grad)
    return Case('loss', 'image-' + lc.case_id(case), lambda lib: [lib.arvae_recon_ws_floats(int(np.prod(case[1])))], run)


def _token_case(case):
    def run(dev):
        from arvae_amd import ops
        inp = lc.token_inputs(case)
        w, tgt = _to(inp['w'], dev, True), _to(inp['tgt'], dev)
        loss, acc = ops.token_recon(w, tgt)
        loss.backward()
        return dict(loss=loss.detach(), acc=acc, dw=w.grad)
    return Case('loss', 'token-' + lc.case_id(case), lambda lib: [lib.arvae_recon_ws_floats(case[0][0])], run)


# =====================================================================================================================
# sequence side
# =====================================================================================================================
EMBED_PICKS = [sq.EMBED_CASES[0],                                            # the smallest
               _first(sq.EMBED_CASES, lambda c: c[0] == 10 and c[2] == (86, 24) and c[1] == 63),      # narrow rows: embed_bwd_partial_kernel
               _first(sq.EMBED_CASES, lambda c: c[0] == 129 and c[2] == (1, 5)),                      # wide rows, 11 empty position groups
               _first(sq.EMBED_CASES, lambda c: c[0] == 132 and c[2] == (86, 24))]                    # wide rows, overwritten table
PROJECTION_PICKS = [sq.TICK_PROJECTION_CASES[0],                             # hidden 32, batch 1
                    _first(sq.TICK_PROJECTION_CASES, lambda c: c[1] == 85 and c[2] == 62)]            # the LDS bound passes by one


def _embed_case(case):
    dim, vocab, (batch, steps), _tm, _acc, _pattern = case

    def run(dev):
        from arvae_amd import ops
        inp = sq.embed_inputs(case)
        idx, g = _to(inp['idx'], dev), _to(inp['g'], dev)
        table = _to(inp['table'], dev, True)
        if inp['acc']:
            table.grad = _to(inp['old'], dev).clone()
        out = ops.embed(idx, table, time_major=bool(inp['tm']))
        out.backward(g.view(out.shape))
        return dict(out=out.detach(), dtable=table.grad)
    return Case('sequence', 'embed-' + sq.case_id(case), lambda lib: [lib.arvae_embed_bwd_ws_floats(batch, steps, dim, vocab)], run)


def _projection_case(case):
    hidden, batch, vocab, _preset = case

    def sizes(lib):
        from arvae_amd import ops
        d = ops.Link.dense(sq.PROJ_EMB + hidden, 3 * hidden).desc(vocab + 1 + sq.PROJ_BEATS * batch)
        return [lib.arvae_tick_gi_bwd_ws_floats(vocab, 3 * hidden), lib.arvae_link_wgrad_ws_floats(ctypes.byref(d)),
                lib.arvae_channel_sum_ws_floats(vocab + 1, 3 * hidden)]

    def run(dev):
        from arvae_amd import ops
        inp = sq.tick_projection_inputs(case)
        p = {k: _to(inp[k], dev, True) for k in ('table', 'x0', 'beat_emb', 'w_ih', 'b_ih')}
        for k in ('table', 'x0', 'w_ih', 'b_ih'):
            if inp['preset']:
                p[k].grad = _to(inp['old_' + k], dev).clone()
        gi = ops.tick_input_projection(p['table'], p['x0'], p['beat_emb'], p['w_ih'], p['b_ih'], _to(inp['tokens'], dev), inp['beats'], inp['tpb'])
        gi.backward(_to(inp['dgi'], dev).view(gi.shape))
        assert not ops._WGRAD_QUEUE
        return dict(gi=gi.detach(), **{'d_' + k: v.grad for k, v in p.items()})
    return Case('sequence', 'tick_projection-' + sq.case_id(case), sizes, run)


GRU_PROBLEM = (32, 6, 21)                                        # hidden 32, 6 steps, 21 rows: outputs only, they get bands too


def _gru_case():
    hid, steps, rows = GRU_PROBLEM

    def sizes(lib):
        from arvae_amd import ops
        return [lib.arvae_link_wgrad_ws_floats(ctypes.byref(ops.Link.dense(hid, 3 * hid).desc(steps * rows)))]

    def run(dev):
        """gru_cases.problem through ops.dense and ONE ops.gru_sequence launch of four sequences, as test_gru_recurrences_float64 runs it"""
        from arvae_amd import ops
        p = gru_cases.problem(hid, steps, rows)
        dirs, leaves = [], []
        for k, gru in enumerate(p['layers']):
            prm = {n: v.detach().clone().to(dev).requires_grad_(True) for n, v in gru.named_parameters()}
            xd, hd = p['x'][k].to(dev).requires_grad_(True), p['h0'][k].to(dev).requires_grad_(True)
            for d, suf in enumerate(('', '_reverse')):
                gi = ops.dense(xd.view(steps * rows, gru_cases.FIN), prm['weight_ih_l0' + suf], prm['bias_ih_l0' + suf],
                               ops.Link.dense(gru_cases.FIN, 3 * hid), 0).view(steps, rows, 3 * hid)
                dirs.append((gi, prm['weight_hh_l0' + suf], prm['bias_hh_l0' + suf], hd[d], gru_cases.REVERSE[2 * k + d]))
            leaves.append((prm, xd, hd))
        yd, fin = ops.gru_sequence(steps, dirs)
        ((yd * torch.cat(list(p['gy']), 2).to(dev)).sum() + (fin * torch.cat(list(p['gfin']), 1).to(dev)).sum()).backward()
        out = dict(y=yd.detach(), fin=fin.detach())
        for k, (prm, xd, hd) in enumerate(leaves):
            out.update({f'dx{k}': xd.grad, f'dh0_{k}': hd.grad})
            out.update({f'd{n}[{k}]': v.grad for n, v in prm.items()})
        return out
    return Case('sequence', f'gru_sequence-H{hid}-T{steps}-R{rows}', sizes, run)


# =====================================================================================================================
# one-launch tick decoders and beam searches
# =====================================================================================================================
TICK_SHAPES = ((5, 1, 4), (21, 4, 6))                            # (batch, beats, ticks per beat): one beat x 4 ticks; the model's 4 x 6
TICK_SIZES = ((32, 32), (64, 35), (128, 35))                     # (hidden, vocab): vocab <= 16 * (hidden / 16)
BEAM_WIDTH, BEAM_GROUPS, BEAM_PENALTY = 4, 2, 0.5


def _tick_inputs(hid, vocab, batch, beats, tpb, layers):
    """weights as synthetic.synth_tensor draws a model's (the output layer spread as the golden cases spread it), states, the
    beat and note halves of layer 0's input projection, uniforms in (0, 1], a keep-mask per layer boundary, a note plan with
    note 0 always allowed"""
    seed = _seed('tick', hid, vocab, batch, beats, tpb, layers)
    ticks, rows = beats * tpb, beats * batch
    t = {}
    for l in range(layers):
        for n, shape in (('weight_ih', (3 * hid, hid)), ('weight_hh', (3 * hid, hid)), ('bias_ih', (3 * hid,)), ('bias_hh', (3 * hid,))):
            t[f'{n}_l{l}'] = syn.synth_tensor(f'rnn_tick.{n}_l{l}', shape, seed)
        t[f'h0_l{l}'] = np.tanh(syn.normal_noise((rows, hid), seed + 10 + l))
    t['w_out'] = 3.0 * syn.synth_tensor('tick_emb_to_note_emb.0.weight', (vocab, hid), seed)
    t['b_out'] = syn.synth_tensor('tick_emb_to_note_emb.0.bias', (vocab,), seed) + np.float32(0.5)
    t['gib'] = 0.5 * syn.normal_noise((rows, 3 * hid), seed + 20)
    t['ptab'] = 0.5 * syn.normal_noise((vocab + 1, 3 * hid), seed + 21)
    rs = np.random.RandomState(seed + 22)
    t['uniforms'] = np.clip(1.0 - rs.random_sample((batch, ticks)), 2.0 ** -32, 1.0).astype(np.float32)
    t['mask'] = np.stack(syn.dropout_masks([(ticks, batch, hid)] * max(layers - 1, 1), seed + 23))
    plan = syn.dropout_masks([(batch, ticks, vocab)], seed + 24)[0]
    plan[..., 0] = 1
    t['plan'] = plan
    return t


def _tick_sizes(hid, layers=2):
    if layers == 2:
        return lambda lib: [lib.arvae_tick_free_run_ws_floats(hid)]
    return lambda lib: [lib.arvae_tick_free_run_layers_ws_floats(hid, layers)]


def _tick_case(form, hid, vocab, shape):
    batch, beats, tpb = shape
    name = f'tick_free_run-{form}-H{hid}-V{vocab}-B{batch}-{beats}x{tpb}'

    def run(dev):
        from arvae_amd import ops
        assert ops.tick_free_run_supported(hid, vocab)
        d = {k: _to(v, dev) for k, v in _tick_inputs(hid, vocab, batch, beats, tpb, 2).items()}
        weights = (d['weight_hh_l0'], d['bias_hh_l0'], d['weight_ih_l1'], d['bias_ih_l1'], d['weight_hh_l1'], d['bias_hh_l1'], d['w_out'], d['b_out'])
        args = (weights, d['h0_l0'], d['h0_l1'], d['gib'], d['ptab'])
        if form == 'argmax':
            tok = ops.tick_free_run(*args, None, 1.0, batch, beats, tpb)
        elif form == 'argmax_masked':
            tok = ops.tick_free_run(*args, d['mask'][0].contiguous(), 2.0, batch, beats, tpb)
        elif form == 'uniforms':
            tok = ops.tick_free_run(*args, None, 1.0, batch, beats, tpb, uniforms=d['uniforms'], temperature=0.8)
        elif form == 'filtered':
            tok = ops.tick_free_run_filtered(*args, batch, beats, tpb, d['uniforms'], 0.8, top_k=5, top_p=0.9)
        else:
            tok = ops.tick_free_run_planned(*args, batch, beats, tpb, d['uniforms'], d['plan'], 0.8, top_k=5, top_p=0.9)
        return dict(tokens=tok, _keep=d)
    return Case('tick_decoders', name, _tick_sizes(hid), run)


def _tick_layers_case(form, hid, vocab, layers, shape):
    batch, beats, tpb = shape
    name = f'tick_free_run_layers-{form}-L{layers}-H{hid}-V{vocab}-B{batch}-{beats}x{tpb}'

    def run(dev):
        from arvae_amd import ops
        assert ops.tick_free_run_layers_supported(hid, vocab, layers)
        d = {k: _to(v, dev) for k, v in _tick_inputs(hid, vocab, batch, beats, tpb, layers).items()}
        cells = [(d[f'weight_ih_l{l}'], d[f'weight_hh_l{l}'], d[f'bias_ih_l{l}'], d[f'bias_hh_l{l}']) for l in range(layers)]
        h0 = [d[f'h0_l{l}'] for l in range(layers)]
        args = (cells, d['w_out'], d['b_out'], h0, d['gib'], d['ptab'])
        if form == 'argmax':
            mask = d['mask'].contiguous() if layers > 1 else None
            tok = ops.tick_free_run_layers(*args, mask, 2.0, batch, beats, tpb)
        elif form == 'uniforms':
            tok = ops.tick_free_run_layers(*args, None, 1.0, batch, beats, tpb, uniforms=d['uniforms'], temperature=0.8)
        elif form == 'filtered':
            tok = ops.tick_free_run_layers_filtered(*args, batch, beats, tpb, d['uniforms'], 0.8, top_k=5, top_p=0.9)
        else:
            tok = ops.tick_free_run_layers_planned(*args, batch, beats, tpb, d['uniforms'], d['plan'], 0.8, top_k=5, top_p=0.9)
        return dict(tokens=tok, _keep=d)
    return Case('tick_decoders', name, _tick_sizes(hid, layers), run)


def _beam_case(form, hid, vocab, shape):
    batch, beats, tpb = shape
    name = f'tick_beam_search-{form}-H{hid}-V{vocab}-B{batch}-{beats}x{tpb}'
    names = ('parents', 'tokens', 'scores_hist', 'sequences', 'scores', 'log_probs')

    def run(dev):
        from arvae_amd import ops
        assert ops.tick_beam_search_groups_supported(hid, vocab, BEAM_WIDTH, BEAM_GROUPS)
        d = {k: _to(v, dev) for k, v in _tick_inputs(hid, vocab, batch, beats, tpb, 2).items()}
        weights = (d['weight_hh_l0'], d['bias_hh_l0'], d['weight_ih_l1'], d['bias_ih_l1'], d['weight_hh_l1'], d['bias_hh_l1'], d['w_out'], d['b_out'])
        args = (weights, d['h0_l0'], d['h0_l1'], d['gib'], d['ptab'], batch, beats, tpb, BEAM_WIDTH)
        if form == 'plain':
            got = ops.tick_beam_search(*args)
        elif form == 'planned':
            got = ops.tick_beam_search_planned(*args, d['plan'])
        else:
            got = ops.tick_beam_search_groups(*args, BEAM_GROUPS, BEAM_PENALTY, d['plan'])
        return dict(zip(names, got), _keep=d)
    return Case('tick_decoders', name, lambda lib: [lib.arvae_tick_beam_search_ws_floats(hid)], run)


def _tick_cases():
    """every form at hidden 32, 64 and 128 where the library offers it (the *_supported predicates; tick_free_run_layers is offered
    for 1, 3 and 4 layers -- two layers are tick_free_run itself --, and not at hidden 128 with 3 or 4: DESIGN.md section 7)"""
    out = []
    for hid, vocab in TICK_SIZES:
        for shape in TICK_SHAPES:
            for form in ('argmax', 'uniforms', 'filtered', 'planned'):
                out.append(_tick_case(form, hid, vocab, shape))
            for form in ('plain', 'planned', 'groups'):
                out.append(_beam_case(form, hid, vocab, shape))
        out.append(_tick_case('argmax_masked', hid, vocab, TICK_SHAPES[1]))
        for layers in (1, 3):
            if hid == 128 and layers >= 3:
                continue
            for shape in TICK_SHAPES:
                for form in ('argmax', 'uniforms'):
                    out.append(_tick_layers_case(form, hid, vocab, layers, shape))
            for form in ('filtered', 'planned'):
                out.append(_tick_layers_case(form, hid, vocab, layers, TICK_SHAPES[1]))
    return out


# =====================================================================================================================
# classifier, KSG
# =====================================================================================================================
RESNET_FC_BIAS_PAD = 2                                           # floats behind the 10 fc biases at the end of the prepared block
EXCEPTIONS += [(f'classify-n{n}', 'prep', 'ops.py:1964 (resnet18_prepare)',
                'resnet18.hip:326 sizes the fc bias as 12 floats (10, padded to a 16-byte multiple), resnet18.hip:459 copies the 10 biases and '
                'resnet18.hip:294 reads fc_b[0..9] only: the last two floats of the prepared block are a pad nobody writes or reads')
               for n in (1, 3)]


@functools.lru_cache(maxsize=None)
def _resnet_fixture():
    return resnet_ref.Fixture(n=3)                               # (made once: three images, the head centred on them)


def _classifier_case(n):
    def run(dev):
        from arvae_amd.mnist_resnet import MnistResNet
        fx = _resnet_fixture()
        model = MnistResNet()
        model.load_state_dict(fx.sd)
        model.to(dev).eval()
        logits, probs, pred = model.classify(_to(fx.x[:n], dev))      # a fresh model: the preparation runs inside the call
        prep = model._prep                                            # (whole: EXCEPTIONS; all but the bias pad: compared)
        return dict(logits=logits, probs=probs, pred=pred, prep=prep, prep_body=prep[:-RESNET_FC_BIAS_PAD], _keep=model)
    return Case('classifier', f'classify-n{n}', lambda lib: [lib.arvae_resnet18_ws_floats(n), lib.arvae_resnet18_prep_floats()], run)


KSG_N, KSG_K = 301, 3


def _ksg_inputs():
    from arvae_amd import evaluation as ev
    codes, attrs, _ = syn.eval_metric_inputs('small', 1)
    return ev.prepare_inputs(codes[:KSG_N], attrs[:KSG_N, 0], np.random.RandomState(2))


def _ksg_case():
    def run(dev):
        from arvae_amd import evaluation as ev
        xp, yp = _ksg_inputs()
        mi, radius, nx, ny = ev.ksg_mi(_to(xp.T, dev), _to(yp.astype(np.float64), dev), KSG_K, with_details=True)
        return dict(mi=mi, radius=radius, nx=nx, ny=ny)
    return Case('ksg', f'ksg_mi-n{KSG_N}-k{KSG_K}', lambda lib: [lib.arvae_ksg_ws_bytes(KSG_N, _ksg_inputs()[0].shape[1])], run)


# =====================================================================================================================
# whole-model executors, through the trainers
# =====================================================================================================================
class DspritesDataset:
    pass


class MorphoMnistDataset:
    pass


class FolkDataset:
    """the attributes MeasureVAE / MeasureVAETrainer read from the reference's FolkNBarDataset"""
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


def _image_trainer(kind):
    from arvae_amd.image_vae import DspritesVAE, MnistVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    from oracle import image_vae as o_vae
    state = syn.synth_state(o_vae.SHAPES[kind], 9 if kind == 'dsprites' else 3, 1.6 if kind == 'dsprites' else 0.7)
    model = DspritesVAE() if kind == 'dsprites' else MnistVAE()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    dims = (1, 2, 3, 4, 5) if kind == 'dsprites' else (1, 2, 3, 4, 5, 6)
    beta = 4.0 if kind == 'dsprites' else 1.0
    trainer = ImageVAETrainer(DspritesDataset() if kind == 'dsprites' else MorphoMnistDataset(), model, lr=1e-4, reg_type=('all',),
                              reg_dim=dims, dec_dist='bernoulli', beta=beta, gamma=10.0, capacity=0.0, rand=0, delta=1.0)
    return model, trainer, dims, beta


def _step_results(trainer, model, loss, acc, train):
    """what a step leaves behind: the scalars, the gradient arena (before the update clears it), the weights and moments after
    optimizer.step(), the optimizer's status words"""
    opt = trainer.optimizer
    out = {}
    if train:
        loss.backward()                                          # (a deferred finishing step fills the scalars in here: read them after)
        out['grad_arena'] = opt.grad_arena.detach().clone()
    out.update(loss=loss.detach().clone(), acc=acc.detach().clone())
    out.update({'term_' + k: v.detach().clone() for k, v in trainer.last_terms.items() if v is not None})
    if train:
        trainer.step()
        out.update(params=opt.param_arena.detach().clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone())
    out['status'] = opt.status_words().clone()
    return out


def _image_executor_case(kind, b, train):
    name = f'{kind}-b{b}-{"train_step" if train else "eval_forward"}'

    def sizes(lib):
        from arvae_amd.fused import FusedImageVAE
        model, trainer, dims, beta = _image_trainer(kind)
        return [FusedImageVAE(model, trainer.optimizer, dims, beta, 10.0, 1.0, 'bernoulli')._ws_floats(b)]

    def run(dev):
        from oracle import image_vae as o_vae
        model, trainer, _dims, _beta = _image_trainer(kind)
        trainer.cuda()
        assert trainer.use_fused
        model.train() if train else model.eval()
        x, lab = (syn.dsprites_batch if kind == 'dsprites' else syn.mnist_batch)(b, seed=50 + b)
        model.push_noise(torch.from_numpy(syn.normal_noise((b, o_vae.Z_DIM[kind]), seed=60 + b)))
        if kind == 'mnist' and train:
            masks = syn.dropout_masks([(b,) + s for s in o_vae.MNIST_MASK_SHAPES], 920 + b)
            model.push_dropout_masks([torch.from_numpy(m).permute(0, 2, 3, 1).contiguous() for m in masks])
        trainer.zero_grad()
        with torch.set_grad_enabled(train):
            loss, acc = trainer.loss_and_acc_for_batch((_to(x, dev), _to(lab, dev)), 0, 0, train)
        out = _step_results(trainer, model, loss, acc, train)
        out.update({'out_' + k: v.detach() for k, v in trainer.last_outputs.items()})
        out['_keep'] = (model, trainer)
        return out
    return Case(EXECUTOR_FAMILY, name, sizes, run)


MEASURE_HIDDEN, MEASURE_Z, MEASURE_DROPOUT = 64, 32, 0.5


def _measure_trainer(dropout):
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    from oracle import measure_vae as o_mvae
    state = syn.synth_state(o_mvae.shapes(hid=MEASURE_HIDDEN, zdim=MEASURE_Z), 4)
    state['decoder.tick_emb_to_note_emb.0.bias'] = state['decoder.tick_emb_to_note_emb.0.bias'] + np.float32(0.5)
    state['decoder.tick_emb_to_note_emb.0.weight'] = state['decoder.tick_emb_to_note_emb.0.weight'] * np.float32(3.0)
    ds = FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, MEASURE_HIDDEN, dropout, MEASURE_Z, 2, MEASURE_HIDDEN, dropout, False, 'folk')
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0, capacity=0.0, rand=0,
                                delta=10.0)
    return model, trainer


def _measure_executor_case(b, teacher, train):
    name = f'measure-b{b}-{"teacher_forced" if teacher else "free_running"}-{"train_step" if train else "eval_forward"}'

    def sizes(lib):
        from arvae_amd.fused_measure import FusedMeasureVAE
        model, trainer = _measure_trainer(MEASURE_DROPOUT)
        assert FusedMeasureVAE.supports(model, trainer.optimizer, (0, 1, 2, 3)) is None
        return [FusedMeasureVAE(model, trainer.optimizer, (0, 1, 2, 3), 0.001, 1.0, 10.0)._ws_floats(b)]

    def run(dev):
        model, trainer = _measure_trainer(MEASURE_DROPOUT)
        trainer.cuda()
        model.train() if train else model.eval()
        model.decoder.teacher_forcing_prob = 2.0 if teacher else -1.0
        h = MEASURE_HIDDEN
        model.push_noise(torch.from_numpy(syn.normal_noise((b, MEASURE_Z), seed=1 if teacher else 2)))
        if train:                                                # the HIP queues take (T, B, H) uint8
            m_enc, m_beat, m_tick = syn.dropout_masks([(b, 24, 2 * h), (b, 4, h), (b, 24, h)], 31, MEASURE_DROPOUT)
            model.encoder.push_dropout_mask(_to(m_enc.transpose(1, 0, 2), dev))
            model.decoder.push_dropout_masks(_to(m_beat.transpose(1, 0, 2), dev), _to(m_tick.transpose(1, 0, 2), dev))
        st = _to(syn.measure_batch(b, seed=5), dev)
        trainer.zero_grad()
        assert trainer.fused_executor(st) is not None            # the executor takes this step, not the per-layer path
        with torch.set_grad_enabled(train):
            loss, acc = trainer.loss_and_acc_for_batch((st, st), 0, 0, train)
        out = _step_results(trainer, model, loss, acc, train)
        out['_keep'] = (model, trainer)
        return out
    return Case(EXECUTOR_FAMILY, name, sizes, run)


def _executor_cases():
    return [_image_executor_case('dsprites', 3, True), _image_executor_case('dsprites', 37, True), _image_executor_case('dsprites', 37, False),
            _image_executor_case('mnist', 37, True), _image_executor_case('mnist', 37, False),
            _measure_executor_case(21, True, True), _measure_executor_case(21, False, True), _measure_executor_case(21, False, False)]


# =====================================================================================================================
# the table
# =====================================================================================================================
def _build():
    cases = _conv32_cases() + _conv64_cases() + [_single_channel_case(c) for c in _single_channel_selection()]
    cases += [_channel_sum_case(r, c) for r in CHANNEL_SUM_ROWS for c in CHANNEL_SUM_CHANNELS] + [_channel_sum_case(17, 64, folded=True)]
    wide = [c for c in sp.DENSE_WIDE if c[0] in (5, 1100)]
    cases += [_wide_dense_case(c, mode) for c in wide for mode in (0, 1, 2)]
    cases += [_dense_case(c, False) for c in DENSE_LONG] + [_dense_case(DENSE_SMALL, True)]
    cases += [_reg_case(c) for c in REG_PICKS] + [_image_case(c) for c in IMAGE_PICKS] + [_token_case(c) for c in TOKEN_PICKS]
    cases += [_embed_case(c) for c in EMBED_PICKS] + [_projection_case(c) for c in PROJECTION_PICKS] + [_gru_case()]
    cases += _tick_cases() + [_classifier_case(1), _classifier_case(3), _ksg_case()] + _executor_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}

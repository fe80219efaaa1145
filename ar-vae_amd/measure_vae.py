"""MeasureVAE (GRU encoder + hierarchical GRU decoder over 24-tick measures) on the HIP kernels.

Same class names, constructor arguments, forward contract and state_dict keys as the reference
(measurevae/encoder.py:8-124, measurevae/decoder.py:7-51,309-525, measurevae/measure_vae.py:11-131):
    MeasureVAE.forward(score, metadata, train) -> (weights (B,24,V), samples (B,1,24), z_dist, prior_dist, z_tilde, z_prior)
Every GRU layer runs as whole-sequence launches (csrc/gru_seq.hip: all time steps of a layer, both directions, in one
kernel forward and one backward; input projections and weight gradients as whole-sequence GEMMs); the free-running
decoder gets its tokens from one more launch.  Any layer count >= 1 (nn.GRU(num_layers=L): layer k > 0 reads layer k-1's outputs,
dropout between layers only); the two-layer stacks of the reference's defaults keep their own one-launch tick kernel.  Hidden sizes other than 32 / 64 / 128 (or ARVAE_GRU_STEPWISE=1) fall back
to one launch per GRU cell and time step (csrc/sequence.hip + the dense kernels).  autograd only chains the launches.
"""
import math
import numbers
import os
from collections import deque

import torch
from torch import distributions, nn

from . import ops
from .model import LayerStack, Model, ParamLayer
from .ops import ACT_NONE, ACT_RELU, ACT_SELU, Link


class GRUParams(nn.Module):
    """Parameters of an nn.GRU under torch's names (weight_ih_l0, weight_hh_l0_reverse, ...)."""

    def __init__(self, input_size, hidden_size, num_layers, bidirectional):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.num_directions = 2 if bidirectional else 1
        bound = 1.0 / (hidden_size ** 0.5)
        for layer in range(num_layers):
            in_l = input_size if layer == 0 else hidden_size * self.num_directions
            for suf in ([''] + (['_reverse'] if bidirectional else [])):
                for name, shape in ((f'weight_ih_l{layer}{suf}', (3 * hidden_size, in_l)),
                                    (f'weight_hh_l{layer}{suf}', (3 * hidden_size, hidden_size)),
                                    (f'bias_ih_l{layer}{suf}', (3 * hidden_size,)),
                                    (f'bias_hh_l{layer}{suf}', (3 * hidden_size,))):
                    p = nn.Parameter(torch.empty(*shape))
                    nn.init.uniform_(p, -bound, bound)
                    self.register_parameter(name, p)

    def cell(self, layer, suffix=''):
        g = lambda n: getattr(self, f'{n}_l{layer}{suffix}')
        return g('weight_ih'), g('weight_hh'), g('bias_ih'), g('bias_hh')


class Embedding(nn.Module):
    def __init__(self, num, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(num, dim))


def _dense_layer(fin, fout):
    return LayerStack([(0, ParamLayer((fout, fin), fout, fin))])


def _lin(x, layer, act):
    w = layer.weight
    return ops.dense(x, w, layer.bias, Link.dense(w.shape[1], w.shape[0]), act)


def _gru_step(x_proj, h, w_hh, b_hh):
    """one GRU time step given the input projection gi = W_ih x + b_ih."""
    gh = ops.dense(h, w_hh, b_hh, Link.dense(w_hh.shape[1], w_hh.shape[0]), ACT_NONE)
    return ops.gru_gates(x_proj, gh, h)


def _split_layers(flat, hidden, layers):
    """(R, layers*H) -> the `layers` initial states (R, H): view(R, layers, H).transpose(0, 1) of decoder.py:388-406"""
    parts = []
    for _ in range(layers - 1):
        head, flat = ops.split_cols(flat, hidden)
        parts.append(head)
    return parts + [flat]


def _boundary_masks(mask, layers, inner, what):
    """an explicit keep-mask as the list of its layers-1 boundaries' masks, each of shape `inner`: (layers-1, *inner), or at two
    layers also the bare `inner` of the one boundary"""
    if mask is not None and layers == 2 and tuple(mask.shape) == tuple(inner):
        return [mask]
    if mask is None or tuple(mask.shape) != (layers - 1,) + tuple(inner):
        got = None if mask is None else tuple(mask.shape)
        raise ValueError(f'{what} keep-mask must be {(layers - 1,) + tuple(inner)} (one per layer boundary), got {got}')
    return list(torch.unbind(mask, 0))


def _use_sequence_kernels(hidden):
    """whole-sequence GRU calls when the hidden size is built: csrc/gru_seq.hip (32, 64, 128: resident weights, one launch) or
    csrc/gru_wide.hip (256, 512: streamed weights, one launch per step inside one call).  ARVAE_GRU_STEPWISE=1 keeps the
    dense + gates launch pair per time step (A/B measurements, and the only path for other hidden sizes)."""
    return os.environ.get('ARVAE_GRU_STEPWISE', '0') != '1' and (ops.gru_sequence_supported(hidden) or
                                                                ops.gru_sequence_wide_supported(hidden))


class Encoder(Model):
    def __init__(self, note_embedding_dim, rnn_hidden_size, num_layers, num_notes, dropout, bidirectional, z_dim,
                 rnn_class=nn.GRU):
        super().__init__()
        if not bidirectional:
            raise NotImplementedError('the HIP encoder implements the reference configuration: a bidirectional GRU')
        if num_layers < 1:
            raise ValueError('num_layers must be at least 1')
        self.bidirectional, self.num_directions = bidirectional, 2
        self.note_embedding_dim, self.num_layers = note_embedding_dim, num_layers
        self.rnn_hidden_size, self.z_dim, self.dropout, self.rnn_class = rnn_hidden_size, z_dim, dropout, rnn_class
        self.num_notes = num_notes
        self.lstm = GRUParams(note_embedding_dim, rnn_hidden_size, num_layers, bidirectional)
        self.note_embedding_layer = Embedding(num_notes, note_embedding_dim)
        feat = rnn_hidden_size * 2 * num_layers
        self.linear_mean = LayerStack([(0, ParamLayer((rnn_hidden_size * 2, feat), rnn_hidden_size * 2, feat)),
                                       (2, ParamLayer((z_dim, rnn_hidden_size * 2), z_dim, rnn_hidden_size * 2))])
        self.linear_log_std = LayerStack([(0, ParamLayer((rnn_hidden_size * 2, feat), rnn_hidden_size * 2, feat)),
                                          (2, ParamLayer((z_dim, rnn_hidden_size * 2), z_dim, rnn_hidden_size * 2))])
        self.xavier_initialization()
        self._mask_queue = deque()
        self._eps_queue = deque()

    def __repr__(self):
        return (f'Encoder({self.note_embedding_dim},{self.rnn_class},{self.num_layers},{self.rnn_hidden_size},'
                f'{self.dropout},{self.bidirectional},{self.z_dim},)')

    def push_dropout_mask(self, mask):
        """explicit keep-masks (num_layers - 1, 24, B, 2H) uint8 for the outputs of every layer but the last (parity runs); with two
        layers also (24, B, 2H).  A one-layer GRU has no boundary to drop at: refused."""
        if self.num_layers == 1:
            raise ValueError('a one-layer GRU has no inter-layer dropout: there is no mask to push')
        self._mask_queue.append(mask)

    def embed_forward(self, score_tensor):
        return ops.embed(score_tensor, self.note_embedding_layer.weight)

    def _layer(self, seq, layer):
        """seq: list of T tensors (B, in) -> (list of T (B, 2H), [final fwd, final rev])."""
        steps, b = len(seq), seq[0].shape[0]
        x_all = torch.cat(seq, 0)                                    # (T*B, in), time-major rows
        outs, finals = [], []
        for suffix in ('', '_reverse'):
            w_ih, w_hh, b_ih, b_hh = self.lstm.cell(layer, suffix)
            gi_all = ops.dense(x_all, w_ih, b_ih, Link.dense(w_ih.shape[1], w_ih.shape[0]), ACT_NONE)
            gi = torch.unbind(gi_all.view(steps, b, -1), 0)
            h = torch.zeros(b, self.rnn_hidden_size, device=x_all.device)
            hs = [None] * steps
            for t in (range(steps) if suffix == '' else range(steps - 1, -1, -1)):
                h = _gru_step(gi[t], h, w_hh, b_hh)
                hs[t] = h
            outs.append(hs)
            finals.append(h)
        return [ops.concat_cols(f, r) for f, r in zip(*outs)], finals

    def push_noise(self, eps):
        """use `eps` (B, z_dim) for the next reparameterised sample instead of drawing it."""
        self._eps_queue.append(eps)

    static_eps = None                                        # tests: fixed noise buffer for eager-vs-graph comparisons

    def forward(self, score_tensor):
        """score (B, 24) int64 -> Normal(mu, exp(log_std)); the reparameterised sample computed by the same
        fused kernel travels with the distribution object (z_dist._arvae_sample)."""
        if ops.checks_enabled():                             # the reference's NaN scan of the weights (encoder.py:101-106)
            ops.check_finite([p for n, p in self.named_parameters() if 'weight' in n], 'Encoder')
        mu, log_std = self.encode_params(score_tensor)
        if self._eps_queue:
            eps = self._eps_queue.popleft().to(mu.device, torch.float32).contiguous()
        elif self.static_eps is not None:                    # a device buffer read at run time (visible to a captured graph)
            eps = self.static_eps
        else:
            eps = ops.normal_noise(mu.shape, mu.device)
        sigma, z = ops.latent_head(mu, log_std, eps)
        z_dist = distributions.Normal(loc=mu, scale=sigma, validate_args=False)
        z_dist._arvae_sample = z
        return z_dist

    def _layer_sequence(self, x_all, steps, b, layer):
        """x_all (T*B, in), time-major rows -> (T, B, 2H): both directions of one layer in one sequence launch."""
        wf, whf, bf, bhf = self.lstm.cell(layer, '')
        wr, whr, br, bhr = self.lstm.cell(layer, '_reverse')
        gi_all = ops.dense_pair(x_all, wf, bf, wr, br)           # (T*B, 2 * 3H) when the two projections are adjacent in memory
        if gi_all is not None:
            return ops.gru_sequence(steps, [(None, whf, bhf, None, False), (None, whr, bhr, None, True)],
                                    merged_gi=gi_all.view(steps, b, -1))
        dirs = []
        for suffix in ('', '_reverse'):
            w_ih, w_hh, b_ih, b_hh = self.lstm.cell(layer, suffix)
            gi = ops.dense(x_all, w_ih, b_ih, Link.dense(w_ih.shape[1], w_ih.shape[0]), ACT_NONE)
            dirs.append((gi.view(steps, b, -1), w_hh, b_hh, None, suffix != ''))
        return ops.gru_sequence(steps, dirs)

    def _lookup_fits(self, steps, b):
        return ops.segment_sum_fits(self.num_notes, steps * b)

    def _first_layer_by_lookup(self, score_tensor, steps, b):
        """Layer 0 sees embedded tokens, so its input projection takes only `num_notes` distinct values: P = table W_ih^T + b_ih
        (both directions side by side, num_notes x 6H: one small product) and gi[t, b] = P[score[b, t]] (a lookup, no
        whole-sequence GEMM); backward the per-position gradients are summed per token into dP (a segment sum) and the
        weight / bias / embedding gradients follow from dP on num_notes rows instead of T*B.  The same algebra as
        encoder.py:111-114 (embedding, then nn.GRU's W_ih x + b_ih), re-associated.  -> (out, finals) or (None, None) when the
        two directions' projections are not adjacent in memory (ops.dense_pair)."""
        # the lookup's backward is the wide-row segment sum (csrc/sequence.hip, embed_bwd_wide_kernel): its per-token accumulators
        # and this batch's positions must fit 64 KB of LDS -- the decoder's lookup and FusedMeasureVAE.fits() test the same bound
        if not self._lookup_fits(steps, b):
            return None, None
        wf, whf, bf, bhf = self.lstm.cell(0, '')
        wr, whr, br, bhr = self.lstm.cell(0, '_reverse')
        ptab = ops.dense_pair(self.note_embedding_layer.weight, wf, bf, wr, br)            # (num_notes, 2 * 3H)
        if ptab is None:
            return None, None
        gi_all = ops.embed(score_tensor, ptab, time_major=True)                            # (T, B, 2 * 3H)
        return ops.gru_sequence(steps, [(None, whf, bhf, None, False), (None, whr, bhr, None, True)], merged_gi=gi_all)

    def encode_params(self, score_tensor):
        """-> (mu, log_std)"""
        b, steps = score_tensor.shape
        hid = self.rnn_hidden_size
        # (T, B, E); with the lookup path of layer 0 nothing reads it and autograd drops the launch's backward
        emb = None if _use_sequence_kernels(hid) else ops.embed(score_tensor, self.note_embedding_layer.weight, time_major=True)
        layers = self.num_layers
        dropping = self.training and self.dropout > 0 and layers > 1          # nn.GRU drops between layers only
        masks = None
        if dropping:
            dev = score_tensor.device
            if self._mask_queue:
                masks = _boundary_masks(self._mask_queue.popleft().to(dev), layers, (steps, b, 2 * hid), 'encoder')
            else:                                                # one draw (one Philox offset) per boundary, lowest boundary first
                masks = [ops.keep_mask((steps, b, 2 * hid), self.dropout, dev) for _ in range(layers - 1)]
        if _use_sequence_kernels(hid):
            out0, fin0 = self._first_layer_by_lookup(score_tensor, steps, b)
            if out0 is None:
                emb = ops.embed(score_tensor, self.note_embedding_layer.weight, time_major=True)
                out0, fin0 = self._layer_sequence(emb.view(steps * b, -1), steps, b, 0)
            # h_n of nn.GRU: (layer 0 fwd, layer 0 rev, layer 1 fwd, layer 1 rev, ...), each direction's LAST processed step
            out, hidden = out0, fin0
            for layer in range(1, layers):
                mid = out.view(steps * b, 2 * hid)
                if dropping:
                    mid = ops.dropout_mask(mid, masks[layer - 1].contiguous().view(steps * b, 2 * hid), self.dropout)
                out, fin = self._layer_sequence(mid, steps, b, layer)
                hidden = ops.concat_cols(hidden, fin)
        else:
            seq = list(torch.unbind(emb, 0))
            seq, finals = self._layer(seq, 0)
            hidden = ops.concat_cols(finals[0], finals[1])
            for layer in range(1, layers):
                if dropping:
                    seq = [ops.dropout_mask(s, m, self.dropout) for s, m in zip(seq, torch.unbind(masks[layer - 1].contiguous(), 0))]
                seq, finals = self._layer(seq, layer)
                hidden = ops.concat_cols(hidden, ops.concat_cols(finals[0], finals[1]))
        la, lb = self.linear_mean[0], self.linear_log_std[0]
        both = ops.dense_pair(hidden, la.weight, la.bias, lb.weight, lb.bias, ACT_SELU)      # (B, 2 * 2H) or None
        if both is not None:
            h_mu, h_ls = ops.split_cols(both, la.weight.shape[0])
        else:
            h_mu, h_ls = _lin(hidden, la, ACT_SELU), _lin(hidden, lb, ACT_SELU)
        mu = _lin(h_mu, self.linear_mean[2], ACT_NONE)
        log_std = _lin(h_ls, self.linear_log_std[2], ACT_NONE)
        return mu, log_std


class Decoder(nn.Module):
    def __init__(self, note_embedding_dim, num_notes, z_dim):
        super().__init__()
        self.name = 'DecoderABC'
        self.num_notes, self.note_embedding_dim, self.z_dim = num_notes, note_embedding_dim, z_dim

    def xavier_initialization(self):
        for name, param in self.named_parameters():
            if 'weight' in name:
                nn.init.xavier_normal_(param)


def check_sampling_cuts(top_k, top_p, vocab=None):
    """the one place that knows the cuts' ranges (HierarchicalDecoder.sampling_filter, the command line): top_k None or an integer in
    [1, vocab] (vocab None: no upper end known yet), top_p None or a number in (0, 1].  -> (top_k as int, top_p as float)"""
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral):
            raise TypeError(f'top_k must be an integer, got {type(top_k).__name__}')
        if top_k < 1 or (vocab is not None and top_k > vocab):
            raise ValueError(f'top_k must lie in [1, {"the vocabulary" if vocab is None else vocab}], got {top_k}')
        top_k = int(top_k)
    if top_p is not None:
        if isinstance(top_p, bool) or not isinstance(top_p, numbers.Real):
            raise TypeError(f'top_p must be a number, got {type(top_p).__name__}')
        if not (math.isfinite(top_p) and 0.0 < top_p <= 1.0):
            raise ValueError(f'top_p must lie in (0, 1], got {top_p}')
        top_p = float(top_p)
    return top_k, top_p


class HierarchicalDecoder(Decoder):
    def __init__(self, note_embedding_dim, num_notes, z_dim, num_layers, rnn_hidden_size, dropout, rnn_class=nn.GRU):
        super().__init__(note_embedding_dim, num_notes, z_dim)
        if num_layers < 1:
            raise ValueError('num_layers must be at least 1')
        self.name = 'HierarchicalDecoder'
        self.rnn_class, self.num_layers, self.rnn_hidden_size, self.dropout = rnn_class, num_layers, rnn_hidden_size, dropout
        h = rnn_hidden_size
        self.b_0 = nn.Parameter(torch.zeros(1))
        self.x_0 = nn.Parameter(torch.zeros(note_embedding_dim))
        self.note_embedding_layer = Embedding(num_notes, note_embedding_dim)
        self.z_to_beat_rnn_input = _dense_layer(z_dim, h * num_layers)
        self.beat_rnn_input_dim = 1
        self.rnn_beat = GRUParams(1, h, num_layers, False)
        self.beat_emb_to_tick_rnn_hidden = _dense_layer(h, h * num_layers)
        self.beat_emb_to_tick_rnn_input = _dense_layer(h, h)
        self.rnn_tick = GRUParams(note_embedding_dim + h, h, num_layers, False)
        self.tick_emb_to_note_emb = _dense_layer(h, num_notes)
        self.use_teacher_forcing = True
        self.teacher_forcing_prob = 0.5
        self.sampling = 'argmax'                               # or 'multinomial' (decoder.py:372,431-434,502-505)
        self.temperature = 1.0                                 # softmax(probs / temperature); 1 = the reference's softmax(probs)
        self.xavier_initialization()
        self._mask_queue = deque()
        self._uniform_queue = deque()
        self._filter = None                                    # (top_k, top_p, allowed on the device) while `generate` runs with cuts
        self._plan = None                                      # (top_k, top_p, plan (B, 24, V) on the device) while it runs with a note plan

    def __repr__(self):
        return f'{self.name}{self.note_embedding_dim},{self.rnn_class},{self.num_layers},{self.rnn_hidden_size},{self.dropout},)'

    def push_dropout_masks(self, beat_mask, tick_mask):
        """explicit keep-masks (num_layers - 1, 4, B, H) and (num_layers - 1, 24, B, H) uint8 for the hidden states of every layer but
        the last of the beat and the tick RNN; with two layers also (4, B, H) and (24, B, H).  One-layer GRUs have no boundary: refused."""
        if self.num_layers == 1:
            raise ValueError('a one-layer GRU has no inter-layer dropout: there are no masks to push')
        self._mask_queue.append((beat_mask, tick_mask))

    def push_sampling_uniforms(self, u):
        """explicit draws (B, 24) float32 in (0, 1] for the next forward that samples (sampling == 'multinomial', train, not
        teacher-forced): tick t of row b takes the smallest note whose softmax CDF reaches u[b, t]."""
        self._uniform_queue.append(u)

    def _sampling_uniforms(self, b, device):
        """the (B, 24) draws of one sampled forward: the pushed buffer, else ONE launch of the library's generator (one offset)"""
        ticks = 24
        if self._uniform_queue:
            u = self._uniform_queue.popleft().to(device=device, dtype=torch.float32).contiguous()
            if tuple(u.shape) != (b, ticks):
                raise ValueError(f'sampling uniforms must be ({b}, {ticks}), got {tuple(u.shape)}')
            return u
        return ops.philox_uniform((b, ticks), device)

    def hidden_init(self, inp, rnn_type):
        """(B, feats) -> [layer-0 hidden, layer-1 hidden, ...]  (view(B, L, H).transpose(0, 1), decoder.py:388-406)."""
        if rnn_type == 'beat':
            flat = _lin(inp, self.z_to_beat_rnn_input[0], ACT_SELU)
        elif rnn_type == 'tick':
            flat = _lin(inp, self.beat_emb_to_tick_rnn_hidden[0], ACT_SELU)
        else:
            raise ValueError
        return _split_layers(flat, self.rnn_hidden_size, self.num_layers)

    def _stack_step(self, rnn, gi0, h, masks):
        """one time step of the layer stack: h = the layers' states, masks = per boundary a keep-mask (B, H), or None"""
        new = [_gru_step(gi0, h[0], rnn.cell(0)[1], rnn.cell(0)[3])]
        for layer in range(1, self.num_layers):
            mid = ops.dropout_mask(new[-1], masks[layer - 1], self.dropout) if masks is not None else new[-1]
            w_ih, w_hh, b_ih, b_hh = rnn.cell(layer)
            gi = ops.dense(mid, w_ih, b_ih, Link.dense(w_ih.shape[1], w_ih.shape[0]), ACT_NONE)
            new.append(_gru_step(gi, h[layer], w_hh, b_hh))
        return new

    def forward(self, z, score_tensor, train):
        if z.size(1) != self.z_dim or z.size(0) != score_tensor.size(0):
            raise AssertionError('latent / score shape mismatch')
        if ops.checks_enabled():                             # the reference's NaN scan of the weights (decoder.py:420-425)
            ops.check_finite([p for n, p in self.named_parameters() if 'weight' in n], 'Decoder')
        weights, samples = self._forward(z, score_tensor, train)
        if ops.checks_enabled():                             # Decoder.check_index on every fed-back note (decoder.py:30-41)
            ops.check_index(samples, self.num_notes)
        return weights, samples

    def _forward(self, z, score_tensor, train):
        if self.use_teacher_forcing and train:
            teacher_forced = torch.rand(1).item() < self.teacher_forcing_prob       # host coin (decoder.py:427-428)
        else:
            teacher_forced = False
        if self.sampling not in ('argmax', 'multinomial'):
            raise NotImplementedError(f'sampling {self.sampling!r}: argmax and multinomial are implemented')
        if not self.temperature > 0:
            raise ValueError('the sampling temperature must be positive')
        sampling = self.sampling if train else 'argmax'        # decoder.py:431-434
        b = z.size(0)
        uniforms = None                                        # drawn only by a forward that samples: argmax consumes no offset
        if sampling == 'multinomial' and not teacher_forced:
            uniforms = self._sampling_uniforms(b, z.device)
        masks = (None, None)                                   # per RNN: its layers-1 boundaries' keep-masks
        layers, h = self.num_layers, self.rnn_hidden_size
        if self.training and self.dropout > 0 and layers > 1:  # nn.GRU drops between layers only
            if self._mask_queue:
                beat, tick = (m.to(z.device) for m in self._mask_queue.popleft())
                masks = (_boundary_masks(beat, layers, (4, b, h), 'beat'), _boundary_masks(tick, layers, (24, b, h), 'tick'))
            else:
                # per boundary ONE draw (one Philox offset) for the beat (4 steps) and the tick (24 steps) masks, lowest boundary first
                both = [ops.keep_mask((4 + 24, b, h), self.dropout, z.device) for _ in range(layers - 1)]
                masks = ([m[:4] for m in both], [m[4:] for m in both])
        if _use_sequence_kernels(self.rnn_hidden_size):
            beat_out = self.beat_rnn_sequence(z, 4, masks[0])
            return self.tick_rnn_sequence(score_tensor, beat_out, 6, teacher_forced, masks[1], uniforms)
        beat_out = self.forward_beat_rnn(z, 4, masks[0])
        return self.forward_tick_rnn(score_tensor, beat_out, 6, teacher_forced, sampling, masks[1], uniforms)

    def sampling_filter(self, top_k=None, top_p=None, allowed=None):
        """the cuts of `generate`, validated on the host: -> None when none is given, else (top_k or None, top_p or None, allowed as a
        uint8 CPU tensor (V,) or None).  top_k: an int in [1, V]; top_p: a number in (0, 1]; allowed: a mask of V flags (bool or
        0 / 1: tensor, array or sequence) with at least one note allowed."""
        if top_k is None and top_p is None and allowed is None:
            return None
        v = self.num_notes
        top_k, top_p = check_sampling_cuts(top_k, top_p, v)
        if allowed is not None:
            mask = torch.as_tensor(allowed).detach().cpu()
            if mask.dtype == torch.bool:
                mask = mask.to(torch.uint8)
            if mask.dtype.is_floating_point or mask.dtype.is_complex:
                raise TypeError(f'the allowed-note mask must hold flags (bool or 0 / 1 integers), got {mask.dtype}')
            if tuple(mask.shape) != (v,):
                raise ValueError(f'the allowed-note mask must have one flag per note of the vocabulary, shape ({v},), got {tuple(mask.shape)}')
            if bool(((mask != 0) & (mask != 1)).any()):
                raise ValueError('the allowed-note mask must hold flags (0 or 1)')
            if not bool(mask.any()):
                raise ValueError('the allowed-note mask allows no note of the vocabulary')
            allowed = mask.to(torch.uint8).contiguous()
        return top_k, top_p, allowed

    def note_plan(self, plan, batch, allowed=None):
        """a note plan, validated on the host (the one place, as `sampling_filter` is for the cuts): plan[b, t, v] set = note v may be
        emitted for row b at tick t; (24, V) = the same plan for every row, or (B, 24, V); flags (bool or 0 / 1 integers: tensor, array
        or nested sequence).  Intersected with `allowed` (V flags) where given; every tick must keep a note.  A tick with one note
        forces it.  -> uint8 CPU tensor (B, 24, V), or None for no plan -- and for a plan of all ones, which is the call without one."""
        if plan is None:
            return None
        v, ticks = self.num_notes, 24
        mask = torch.as_tensor(plan).detach().cpu()
        if mask.dtype.is_floating_point or mask.dtype.is_complex:
            raise TypeError(f'a note plan must hold flags (bool or 0 / 1 integers), got {mask.dtype}')
        if tuple(mask.shape) == (v,):
            raise ValueError(f'a note plan has one mask per tick, shape ({ticks}, {v}) or ({batch}, {ticks}, {v}); a ({v},) mask for every '
                             f'tick is `allowed`')
        if tuple(mask.shape) not in ((ticks, v), (batch, ticks, v)):
            raise ValueError(f'a note plan must have shape ({ticks}, {v}) or ({batch}, {ticks}, {v}), got {tuple(mask.shape)}')
        if mask.dtype != torch.bool and bool(((mask != 0) & (mask != 1)).any()):
            raise ValueError('a note plan must hold flags (0 or 1)')
        mask = mask != 0
        if bool(mask.all()):
            return None
        flt = self.sampling_filter(None, None, allowed)
        if flt is not None:
            mask = mask & (flt[2] != 0)
        empty = (~mask.any(-1)).nonzero()
        if empty.numel():
            where = tuple(int(i) for i in empty[0])
            raise ValueError(f'the note plan leaves no note at {"tick" if len(where) == 1 else "(row, tick)"} {where if len(where) > 1 else where[0]}'
                             f'{" after the intersection with `allowed`" if flt is not None else ""}')
        return mask.expand(batch, ticks, v).to(torch.uint8).contiguous()

    def generate(self, z, sampling='multinomial', temperature=1.0, uniforms=None, top_k=None, top_p=None, allowed=None, plan=None):
        """Free-running decode of latent codes z (B, z_dim) without autograd and with dropout off: -> (weights (B, 24, V), samples
        (B, 1, 24)).  sampling 'multinomial' draws every fed-back note from softmax(probs / temperature) (uniforms: explicit (B, 24)
        draws in (0, 1], else one launch of the library's generator); 'argmax' feeds the top-1 note back.
        top_k / top_p / allowed (multinomial only; `sampling_filter`): the draw is over the notes that survive -- allowed[v] set, fewer
        than top_k allowed notes ordered before v (descending logit, ties to the lower index), and those notes' share of the softmax
        mass below top_p (the first note always survives); include/arvae_hip.h, arvae_sample_filter_t.  The returned weights are
        the unfiltered logits.
        plan (`note_plan`): the allowed notes per (row, tick), intersected with `allowed`; the rule above with that set at every tick.
        With a plan 'argmax' is accepted too: the allowed note with the largest logit (the top_k = 1 rule; no draw is consumed).  The
        note fed back is the emitted one, forced or chosen."""
        if sampling not in ('argmax', 'multinomial'):
            raise NotImplementedError(f'sampling {sampling!r}: argmax and multinomial are implemented')
        planned = self.note_plan(plan, z.size(0), allowed)
        if planned is not None:
            if sampling == 'argmax' and (top_k is not None or top_p is not None):
                raise ValueError('top_k and top_p cut the multinomial draw: under a plan, argmax takes the best allowed note')
            top_k, top_p = check_sampling_cuts(top_k, top_p, self.num_notes)
            planned = (top_k, top_p, planned.to(z.device))     # the one upload of the call
            top_k = top_p = allowed = None
        flt = self.sampling_filter(top_k, top_p, allowed)
        if flt is not None and sampling != 'multinomial':
            raise ValueError('top_k, top_p and allowed cut the multinomial draw: they need sampling=\'multinomial\'')
        if flt is not None and flt[2] is not None:
            flt = (flt[0], flt[1], flt[2].to(z.device))        # the one upload of the call
        dummy = torch.zeros(z.size(0), 24, dtype=torch.int64, device=z.device)
        saved = (self.sampling, self.temperature, self.use_teacher_forcing, self.training)
        self.sampling, self.temperature, self.use_teacher_forcing = sampling, float(temperature), False
        self.train(False)
        self._filter, self._plan = flt, planned
        try:
            if uniforms is not None and sampling == 'multinomial':
                self.push_sampling_uniforms(uniforms)
            with torch.no_grad():
                return self.forward(z, dummy, sampling == 'multinomial')      # train=True is what lets `sampling` apply
        finally:
            self._filter = self._plan = None
            self.sampling, self.temperature, self.use_teacher_forcing = saved[:3]
            self.train(saved[3])

    # ---- beam search ---------------------------------------------------------------------------------------------
    def _beam_mask(self, beam_width, allowed, device):
        """beam_search's arguments, validated on the host -> (W, the mask uint8 (V,) on `device` or None, the notes it allows)"""
        if isinstance(beam_width, bool) or not isinstance(beam_width, numbers.Integral):
            raise TypeError(f'beam_width must be an integer, got {type(beam_width).__name__}')
        if not 1 <= beam_width <= 16:
            raise ValueError(f'beam_width must lie in [1, 16], got {beam_width}')
        flt = self.sampling_filter(None, None, allowed)
        mask = None if flt is None else flt[2]
        count = self.num_notes if mask is None else int(mask.count_nonzero())
        if beam_width > count:
            raise ValueError(f'beam_width {beam_width} is above the {count} allowed notes: fewer distinct hypotheses exist after the first tick')
        return int(beam_width), (None if mask is None else mask.to(device)), count

    def _eval_no_grad(self, fn):
        """fn() without autograd, with dropout off and teacher forcing on, the decoder's state put back afterwards (as `generate`)"""
        saved = (self.use_teacher_forcing, self.training)
        self.use_teacher_forcing = True
        self.train(False)
        try:
            with torch.no_grad():
                return fn()
        finally:
            self.use_teacher_forcing = saved[0]
            self.train(saved[1])

    def _beats(self, z):
        """-> the beat RNN's outputs (4, B, H)"""
        if _use_sequence_kernels(self.rnn_hidden_size):
            return self.beat_rnn_sequence(z, 4, None)
        return torch.stack(self.forward_beat_rnn(z, 4, None), 0)

    def _teacher_forced_weights(self, beat_out, tokens):
        """the logits (B, 24, V) of the decoder fed `tokens` (B, 24): the existing teacher-forced path"""
        if _use_sequence_kernels(self.rnn_hidden_size):
            return self.tick_rnn_sequence(tokens, beat_out, 6, True)[0]
        return self.forward_tick_rnn(tokens, list(torch.unbind(beat_out, 0)), 6, True, 'argmax')[0]

    def _beam_history(self, beat_out, width, mask, count, plan=None, groups=None):
        """-> (parents (B, 24, W) int32, tokens (B, 24, W) int64, scores (B, 24, W), sequences (B, W, 24) int64, scores (B, W)): one
        launch (csrc/beam_decoder.hip, tick_beam_search_kernel) where it is offered; at hidden 256 / 512 with two layers and up to 128
        notes one call of four launches per tick (csrc/beam_wide.hip, ops.tick_beam_search_wide: plain, planned and grouped alike);
        else tick by tick with the existing dense and gate launches, ops.beam_select and a gather of the states
        (ARVAE_TICK_STEPWISE=1, other layer counts, other hidden sizes, V > 128, and V > 64 below hidden 256).
        plan (B, 24, V) uint8 on the device: the planned forms of both (mask and count are then not read).
        groups (G, penalty): the diverse search (include/arvae_hip.h, "Diverse beam search") -- ops.tick_beam_search_groups where
        offered, else ops.beam_select_groups per tick --, plan then always given (B, 24, V) or one mask (V,); a sixth tensor, the
        log_probs (B, W), is returned."""
        nb, b, hid = beat_out.shape
        layers, vocab = self.num_layers, self.num_notes
        h0, beat_emb = self._tick_restart(beat_out.reshape(nb * b, hid))
        w_ih0, w_hh0, b_ih0, b_hh0 = self.rnn_tick.cell(0)
        out = self.tick_emb_to_note_emb[0]
        stepwise = os.environ.get('ARVAE_TICK_STEPWISE', '0') == '1'
        one_launch = not stepwise and layers == 2 and (ops.tick_beam_search_supported(hid, vocab, width) if groups is None else
                                                       ops.tick_beam_search_groups_supported(hid, vocab, width, groups[0]))
        wide = not stepwise and layers == 2 and not one_launch and ops.tick_beam_search_wide_supported(
            hid, vocab, width, 1 if groups is None else groups[0])
        if one_launch or wide:
            emb_dim = self.note_embedding_dim
            w_note, w_beat = w_ih0[:, :emb_dim].contiguous(), w_ih0[:, emb_dim:].contiguous()
            gib = ops.dense(beat_emb, w_beat, b_ih0, Link.dense(hid, 3 * hid), ACT_NONE)
            table = torch.cat((self.note_embedding_layer.weight, self.x_0[None]), 0)
            ptab = ops.dense(table, w_note, None, Link.dense(emb_dim, 3 * hid), ACT_NONE)
            w_ih1, w_hh1, b_ih1, b_hh1 = self.rnn_tick.cell(1)
            weights = (w_hh0, b_hh0, w_ih1, b_ih1, w_hh1, b_hh1, out.weight, out.bias)
            if wide:
                return ops.tick_beam_search_wide(weights, h0[0].contiguous(), h0[1].contiguous(), gib, ptab, b, nb, 6, width, mask, count,
                                                 plan, groups)
            if groups is not None:
                return ops.tick_beam_search_groups(weights, h0[0].contiguous(), h0[1].contiguous(), gib, ptab, b, nb, 6, width, groups[0],
                                                   groups[1], plan)
            if plan is not None:
                return ops.tick_beam_search_planned(weights, h0[0].contiguous(), h0[1].contiguous(), gib, ptab, b, nb, 6, width, plan)
            return ops.tick_beam_search(weights, h0[0].contiguous(), h0[1].contiguous(), gib, ptab, b, nb, 6, width, mask, count)
        dev = beat_out.device
        rows = torch.arange(b, device=dev).repeat_interleave(width)               # row (code, k) -> code
        base = (torch.arange(b, device=dev) * width)[:, None]
        prev = self.x_0[None].expand(b * width, -1).contiguous()
        scores = torch.zeros(b, width, device=dev)
        logp = torch.zeros(b, width, device=dev)               # (groups only; at tick 0 the first beam of every group is read)
        parents, tokens, hist = [], [], []
        for i in range(nb):
            h = [s[i * b:(i + 1) * b].index_select(0, rows) for s in h0]
            be = beat_emb[i * b:(i + 1) * b].index_select(0, rows)
            for j in range(6):
                gi0 = ops.dense(ops.concat_cols(prev, be), w_ih0, b_ih0, Link.dense(w_ih0.shape[1], w_ih0.shape[0]), ACT_NONE)
                h = self._stack_step(self.rnn_tick, gi0, h, None)
                probs = _lin(h[-1], out, ACT_RELU)
                live = 1 if i == 0 and j == 0 else width
                if groups is not None:
                    par, note, scores, logp = ops.beam_select_groups(probs, scores, logp, min(live, width // groups[0]), groups[0], groups[1],
                                                                     plan, i * 6 + j, nb * 6)
                elif plan is not None:
                    par, note, scores = ops.beam_select_planned(probs, scores, live, plan, i * 6 + j)
                else:
                    par, note, scores = ops.beam_select(probs, scores, live, mask, count)
                src = (base + par.to(torch.int64)).reshape(-1)
                h = [s.index_select(0, src) for s in h]
                prev = ops.embed(note.view(b * width, 1), self.note_embedding_layer.weight).view(b * width, -1)
                parents.append(par), tokens.append(note), hist.append(scores)
        parents, tokens, hist = torch.stack(parents, 1), torch.stack(tokens, 1), torch.stack(hist, 1)
        at = torch.arange(width, device=dev)[None].expand(b, -1)
        seq = []
        for t in range(nb * 6 - 1, -1, -1):                                       # backtracking: a gather per tick
            seq.append(tokens[:, t].gather(1, at))
            at = parents[:, t].to(torch.int64).gather(1, at)
        res = parents, tokens, hist, torch.stack(seq[::-1], 2), scores
        return res if groups is None else res + (logp,)

    def check_beam_groups(self, beam_width, beam_groups, diversity):
        """beam_search's grouping, validated on the host -> (W, G, the penalty)"""
        for name, n in (('beam_width', beam_width), ('beam_groups', beam_groups)):
            if isinstance(n, bool) or not isinstance(n, numbers.Integral):
                raise TypeError(f'{name} must be an integer, got {type(n).__name__}')
        if not 1 <= beam_width <= 16:
            raise ValueError(f'beam_width must lie in [1, 16], got {beam_width}')
        if not 1 <= beam_groups <= beam_width or beam_width % beam_groups:
            raise ValueError(f'beam_groups must lie in [1, beam_width] and divide beam_width = {beam_width}, got {beam_groups}')
        return int(beam_width), int(beam_groups), self._diversity(diversity)

    @staticmethod
    def _diversity(diversity):
        if isinstance(diversity, bool) or not isinstance(diversity, numbers.Real):
            raise TypeError(f'diversity must be a number, got {type(diversity).__name__}')
        if not math.isfinite(diversity) or diversity < 0:
            raise ValueError(f'diversity must be a finite number >= 0, got {diversity}')
        return float(diversity)

    def _diverse_beam_search(self, z, beam_width, beam_groups, diversity, allowed, return_history, plan):
        width, groups, lam = self.check_beam_groups(beam_width, beam_groups, diversity)
        planned = self.note_plan(plan, z.size(0), allowed)
        if planned is None:                                    # one mask for every (row, tick): the plan with both strides 0
            flt = self.sampling_filter(None, None, allowed)
            planned = torch.ones(self.num_notes, dtype=torch.uint8) if flt is None else flt[2]
            count = int(planned.count_nonzero())
            if width // groups > count:
                raise ValueError(f'a group of {width // groups} beams is above the {count} allowed notes: fewer distinct hypotheses '
                                 f'exist after the first tick')
        planned = planned.to(z.device)                         # the one upload of the call

        def run():
            beat_out = self._beats(z)
            parents, tokens, hist, seqs, scores, logp = self._beam_history(beat_out, width, None, None, planned, (groups, lam))
            best = seqs[:, 0].contiguous()
            weights = self._teacher_forced_weights(beat_out, best)
            res = (weights, best[:, None, :], scores[:, 0].contiguous(), seqs, scores, logp)
            return res + ((parents, tokens, hist),) if return_history else res
        return self._eval_no_grad(run)

    def beam_search(self, z, beam_width=4, allowed=None, return_history=False, plan=None, beam_groups=None, diversity=0.0):
        """The beam_width most likely measures of latent codes z (B, z_dim) under the decoder, without autograd and with dropout off
        (include/arvae_hip.h, "Beam search"): -> (weights (B, 24, V), samples (B, 1, 24), scores (B,)) of the best beam -- the weights
        from the whole-sequence kernels evaluated on its tokens --, sequences (B, W, 24) best first and scores (B, W) = their
        log p(x | z) over the allowed notes; return_history=True: also (parents (B, 24, W) int32, tokens (B, 24, W), scores (B, 24, W)).
        allowed: a mask of V flags (`sampling_filter`), at least beam_width of them set.
        plan (`note_plan`): the allowed notes per (row, tick), intersected with `allowed`; the candidates and the softmax of a tick are
        over that set.  Fewer than beam_width hypotheses may then exist (a forced first tick leaves one): the slots without one are
        dead -- score -inf, listed last, their tokens inside the plan -- and beam_width need not be below the allowed notes' count.
        beam_groups=G (dividing beam_width), diversity=L >= 0: the diverse search (include/arvae_hip.h, "Diverse beam search") -- the
        beams in G groups served in order at every tick, a group paying L for every earlier-group beam that has just taken the same
        note -> (weights, samples, score, sequences, scores, log_probs[, history]): sequences group-major and best first within a
        group, scores the ranking scores, log_probs (B, W) the log p(x | z); weights and samples are those of group 0's best beam.
        Without a plan a group's width must not exceed the allowed notes' count.  beam_groups=None is the call without groups."""
        if beam_groups is None:
            if self._diversity(diversity) != 0.0:
                raise ValueError(f'diversity {diversity} needs beam_groups: without groups nothing pays it')
        else:
            return self._diverse_beam_search(z, beam_width, beam_groups, diversity, allowed, return_history, plan)
        planned = self.note_plan(plan, z.size(0), allowed)
        if planned is not None:
            if isinstance(beam_width, bool) or not isinstance(beam_width, numbers.Integral):
                raise TypeError(f'beam_width must be an integer, got {type(beam_width).__name__}')
            if not 1 <= beam_width <= 16:
                raise ValueError(f'beam_width must lie in [1, 16], got {beam_width}')
            width, mask, count = int(beam_width), None, None
            planned = planned.to(z.device)                     # the one upload of the call
        else:
            width, mask, count = self._beam_mask(beam_width, allowed, z.device)

        def run():
            beat_out = self._beats(z)
            parents, tokens, hist, seqs, scores = self._beam_history(beat_out, width, mask, count, planned)
            best = seqs[:, 0].contiguous()
            weights = self._teacher_forced_weights(beat_out, best)
            res = (weights, best[:, None, :], scores[:, 0].contiguous(), seqs, scores)
            return res + ((parents, tokens, hist),) if return_history else res
        return self._eval_no_grad(run)

    def score_tokens(self, z, tokens, allowed=None, plan=None):
        """log p(tokens | z) (B,) under teacher forcing, the softmax over the allowed notes (ops.sequence_log_prob on the
        whole-sequence kernels' weights); tokens (B, 24) or (B, 1, 24) int64.  Without autograd, dropout off.
        plan (`note_plan`): the softmax of a tick over that (row, tick)'s notes; a token outside them gives -inf."""
        planned = self.note_plan(plan, z.size(0), allowed)
        if planned is not None:
            planned = planned.to(z.device)
            tokens = torch.as_tensor(tokens, device=z.device).reshape(z.size(0), 24).to(torch.int64).contiguous()
            return self._eval_no_grad(lambda: ops.sequence_log_prob_planned(
                self._teacher_forced_weights(self._beats(z), tokens).contiguous(), tokens, planned))
        flt = self.sampling_filter(None, None, allowed)
        mask = None if flt is None else flt[2].to(z.device)
        tokens = torch.as_tensor(tokens, device=z.device).reshape(z.size(0), 24).to(torch.int64).contiguous()
        return self._eval_no_grad(lambda: ops.sequence_log_prob(self._teacher_forced_weights(self._beats(z), tokens).contiguous(), tokens, mask))

    # ---- whole-sequence path ------------------------------------------------------------------------------------
    def _stack_sequence(self, rnn, steps, gi0, h0, masks):
        """unidirectional GRU stack over `steps`: gi0 (T, R, 3H) or (R, 3H); h0 = the layers' initial states; masks = per boundary a
        (T*R, H) keep-mask on the lower layer's outputs (nn.GRU's inter-layer dropout), or None.  -> top layer's outputs (T, R, H)"""
        hid = self.rnn_hidden_size
        out, _ = ops.gru_sequence(steps, [(gi0, rnn.cell(0)[1], rnn.cell(0)[3], h0[0], False)], finals=False)
        rows = out.shape[1]
        for layer in range(1, self.num_layers):
            mid = out.view(steps * rows, hid)
            if masks is not None:
                mid = ops.dropout_mask(mid, masks[layer - 1], self.dropout)
            w_ih, w_hh, b_ih, b_hh = rnn.cell(layer)
            gi = ops.dense(mid, w_ih, b_ih, Link.dense(w_ih.shape[1], w_ih.shape[0]), ACT_NONE).view(steps, rows, -1)
            out = ops.gru_sequence(steps, [(gi, w_hh, b_hh, h0[layer], False)], finals=False)[0]
        return out

    def beat_rnn_sequence(self, z, seq_len, mask=None):
        """-> (4, B, H) beat embeddings (decoder.py:436-457)"""
        b = z.size(0)
        h = self.hidden_init(z, 'beat')
        w_ih0, _, b_ih0, _ = self.rnn_beat.cell(0)
        x0 = ops.broadcast_rows(self.b_0, b)
        gi0 = ops.dense(x0, w_ih0, b_ih0, Link.dense(1, w_ih0.shape[0]), ACT_NONE)           # the same input every beat
        m = None if mask is None else [k.contiguous().view(seq_len * b, -1) for k in mask]
        return self._stack_sequence(self.rnn_beat, seq_len, gi0, h, m)

    def _tick_restart(self, bo):
        """beat outputs (4B, H) -> (the tick RNN's initial states per layer, (4B, H) each; the beat embeddings (4B, H))"""
        hid = self.rnn_hidden_size
        la, lb = self.beat_emb_to_tick_rnn_hidden[0], self.beat_emb_to_tick_rnn_input[0]
        both = ops.dense_pair(bo, la.weight, la.bias, lb.weight, lb.bias, ACT_SELU)           # (4B, L H + H) or None
        if both is not None:
            flat, beat_emb = ops.split_cols(both, la.weight.shape[0])
            return _split_layers(flat, hid, self.num_layers), beat_emb
        return self.hidden_init(bo, 'tick'), _lin(bo, lb, ACT_SELU)

    def _tick_lookup_fits(self, positions):
        """the segment sum's LDS holds the vocabulary, x_0 and this batch's ticks; gate rows are multiples of four floats"""
        return (3 * self.rnn_hidden_size) % 4 == 0 and ops.segment_sum_fits(self.num_notes + 1, positions)

    def tick_rnn_sequence(self, score_tensor, beat_out, tick_seq_len, teacher_forced, mask=None, uniforms=None):
        """The tick RNN restarts from a beat-dependent hidden state at every beat (decoder.py:459-525), so given the
        fed-back tokens the four beats are independent 6-step sequences: they run as ONE sequence launch per layer over
        4*B rows (row = beat*B + b).  With teacher forcing the fed-back tokens are the score; otherwise they come from
        the free-running pass `_free_running_tokens` (argmax is not differentiated, decoder.py:506-516), and the same
        graph is then evaluated on those tokens.  uniforms (B, 24): the fed-back notes are drawn (decoder.py:502-505)."""
        nb, b = beat_out.shape[0], beat_out.shape[1]
        hid, steps = self.rnn_hidden_size, tick_seq_len
        ticks = nb * steps
        h0, beat_emb = self._tick_restart(beat_out.view(nb * b, hid))
        m = None
        if mask is not None:                                                                   # per boundary (24, B, H) -> rows (j, beat, b)
            m = [k.view(nb, steps, b, hid).transpose(0, 1).contiguous().view(steps * nb * b, hid) for k in mask]
        if self.use_teacher_forcing and teacher_forced:
            tokens = score_tensor
        else:
            with torch.no_grad():
                tokens = self._free_running_tokens(beat_out.detach(), h0, beat_emb, mask, uniforms)
        w_ih0, _, b_ih0, _ = self.rnn_tick.cell(0)
        if self._tick_lookup_fits(steps * nb * b):
            # layer-0 input projection by lookup: W_ih0 applied once to the vocabulary's embeddings, x_0 and the beat embeddings
            # (num_notes + 1 + 4B rows), each tick's row gathered and added (ops.tick_input_projection)
            gi0 = ops.tick_input_projection(self.note_embedding_layer.weight, self.x_0, beat_emb, w_ih0, b_ih0, tokens, nb, steps)
        else:
            emb_prev = ops.embed(tokens[:, :ticks - 1].contiguous(), self.note_embedding_layer.weight, time_major=True)
            prev = torch.cat((ops.broadcast_rows(self.x_0, b)[None], emb_prev), 0)             # (24, B, E), tick-major
            prev = prev.view(nb, steps, b, -1).transpose(0, 1).reshape(steps * nb * b, -1)     # rows (j, beat, b)
            inp = ops.concat_cols(prev, beat_emb[None].expand(steps, -1, -1).reshape(steps * nb * b, hid))
            gi0 = ops.dense(inp, w_ih0, b_ih0, Link.dense(w_ih0.shape[1], w_ih0.shape[0]), ACT_NONE).view(steps, nb * b, -1)
        top = self._stack_sequence(self.rnn_tick, steps, gi0, h0, m)                           # (6, 4B, H)
        probs = _lin(top.view(steps * nb * b, hid), self.tick_emb_to_note_emb[0], ACT_RELU)
        weights = probs.view(steps, nb, b, -1).permute(2, 1, 0, 3).reshape(b, ticks, -1)       # tick = 6*beat + j
        return weights, tokens[:, None, :]

    def _free_running_tokens(self, beat_out, h0, beat_emb, mask, uniforms=None):
        """feedback pass (no autograd): the tokens the decoder feeds itself, int64 (B, 24): the top-1 note, or with uniforms
        (B, 24) the note drawn from softmax(probs / temperature) at that tick's uniform.  One library call where a decoder kernel is
        built: hidden 32 / 64 / 128 one launch (csrc/tick_decoder.hip), hidden 256 / 512 with two layers three launches per tick
        (csrc/tick_wide.hip); else, and with ARVAE_TICK_STEPWISE=1 (at 256 / 512 also ARVAE_GRU_STEPWISE=1), tick by tick."""
        nb, b = beat_out.shape[0], beat_out.shape[1]
        hid = self.rnn_hidden_size
        w_ih0, w_hh0, b_ih0, b_hh0 = self.rnn_tick.cell(0)
        layers = self.num_layers
        stepwise = os.environ.get('ARVAE_TICK_STEPWISE', '0') == '1'
        one_launch = not stepwise and (ops.tick_free_run_supported(hid, self.num_notes) if layers == 2 else
                                       ops.tick_free_run_layers_supported(hid, self.num_notes, layers))
        flt = self._filter if uniforms is not None else None   # `generate`'s cuts; dropout is off there: no keep-masks
        planned = self._plan                                   # `generate`'s note plan: draws, or with no draws its argmax (top_k = 1)
        if (flt is not None or planned is not None) and mask is not None:
            raise RuntimeError('filtered sampling runs with dropout off')
        if planned is not None:
            top_k, top_p, plan = planned if uniforms is not None else (1, None, planned[2])
            draws = uniforms if uniforms is not None else torch.ones(b, nb * 6, device=beat_out.device)
        # hidden 256 / 512: one call of three launches per tick (csrc/tick_wide.hip), every pick and the masked training form
        wide = (not stepwise and not one_launch and layers == 2 and _use_sequence_kernels(hid) and
                ops.tick_free_run_wide_supported(hid, self.num_notes))
        if one_launch or wide:
            # one launch (csrc/tick_decoder.hip: tick_free_run_h2_kernel for two layers, tick_free_run_layers_kernel otherwise).  W_ih0
            # acts on [previous-note embedding | beat embedding]: the beat half is applied once per beat, the note half once per
            # vocabulary entry (+ x_0).
            emb_dim = self.note_embedding_dim
            w_note, w_beat = w_ih0.detach()[:, :emb_dim].contiguous(), w_ih0.detach()[:, emb_dim:].contiguous()
            gib = ops.dense(beat_emb.detach(), w_beat, b_ih0.detach(), Link.dense(hid, 3 * hid), ACT_NONE)
            table = torch.cat((self.note_embedding_layer.weight.detach(), self.x_0.detach()[None]), 0)
            ptab = ops.dense(table, w_note, None, Link.dense(emb_dim, 3 * hid), ACT_NONE)
            out = self.tick_emb_to_note_emb[0]
            keep_scale = 1.0 / (1.0 - self.dropout)
            if layers == 2:
                w_ih1, w_hh1, b_ih1, b_hh1 = self.rnn_tick.cell(1)
                weights = tuple(t.detach() for t in (w_hh0, b_hh0, w_ih1, b_ih1, w_hh1, b_hh1, out.weight, out.bias))
                if wide:
                    return ops.tick_free_run_wide(weights, h0[0].detach(), h0[1].detach(), gib, ptab, b, nb, 6,
                                                  mask=None if mask is None else mask[0].contiguous(), keep_scale=keep_scale,
                                                  uniforms=draws if planned is not None else uniforms, temperature=self.temperature,
                                                  filter=(top_k, top_p) if planned is not None else flt,
                                                  plan=plan if planned is not None else None)
                if planned is not None:
                    return ops.tick_free_run_planned(weights, h0[0].detach(), h0[1].detach(), gib, ptab, b, nb, 6, draws, plan,
                                                     self.temperature, top_k, top_p)
                if flt is not None:
                    return ops.tick_free_run_filtered(weights, h0[0].detach(), h0[1].detach(), gib, ptab, b, nb, 6, uniforms,
                                                      self.temperature, *flt)
                return ops.tick_free_run(weights, h0[0].detach(), h0[1].detach(), gib, ptab,
                                         None if mask is None else mask[0].contiguous(), keep_scale, b, nb, 6,
                                         uniforms=uniforms, temperature=self.temperature)
            cells = [tuple(t.detach() for t in self.rnn_tick.cell(k)) for k in range(layers)]     # the boundaries' masks: (layers-1, 24, B, H)
            if planned is not None:
                return ops.tick_free_run_layers_planned(cells, out.weight.detach(), out.bias.detach(), [s.detach() for s in h0], gib, ptab,
                                                        b, nb, 6, draws, plan, self.temperature, top_k, top_p)
            if flt is not None:
                return ops.tick_free_run_layers_filtered(cells, out.weight.detach(), out.bias.detach(), [s.detach() for s in h0], gib, ptab,
                                                         b, nb, 6, uniforms, self.temperature, *flt)
            return ops.tick_free_run_layers(cells, out.weight.detach(), out.bias.detach(), [s.detach() for s in h0], gib, ptab,
                                            None if mask is None else torch.stack([k.contiguous() for k in mask], 0),
                                            keep_scale, b, nb, 6, uniforms=uniforms, temperature=self.temperature)
        prev = self.x_0.detach()[None].expand(b, -1).contiguous()
        tokens = []
        for i in range(nb):
            h = [s.detach()[i * b:(i + 1) * b] for s in h0]
            be = beat_emb.detach()[i * b:(i + 1) * b]
            for j in range(6):
                t = i * 6 + j
                gi0 = ops.dense(ops.concat_cols(prev, be), w_ih0, b_ih0, Link.dense(w_ih0.shape[1], w_ih0.shape[0]), ACT_NONE)
                h = self._stack_step(self.rnn_tick, gi0, h, None if mask is None else [k[t].contiguous() for k in mask])
                probs = _lin(h[-1], self.tick_emb_to_note_emb[0], ACT_RELU)
                if planned is not None:
                    idx = ops.row_sample_planned(probs, draws[:, t].contiguous(), plan, t, self.temperature, top_k, top_p)
                elif flt is not None:
                    idx = ops.row_sample_filtered(probs, uniforms[:, t].contiguous(), self.temperature, *flt)
                else:
                    idx = ops.row_argmax(probs) if uniforms is None else ops.row_sample(probs, uniforms[:, t].contiguous(), self.temperature)
                prev = ops.embed(idx.view(b, 1), self.note_embedding_layer.weight).view(b, -1)
                tokens.append(idx)
        return torch.stack(tokens, 1)

    def forward_beat_rnn(self, z, seq_len, mask=None):
        b = z.size(0)
        h = self.hidden_init(z, 'beat')
        w_ih0, _, b_ih0, _ = self.rnn_beat.cell(0)
        x0 = ops.broadcast_rows(self.b_0, b)                               # constant input b_0 for every beat
        gi0 = ops.dense(x0, w_ih0, b_ih0, Link.dense(1, w_ih0.shape[0]), ACT_NONE)
        out = []
        for i in range(seq_len):
            h = self._stack_step(self.rnn_beat, gi0, h, None if mask is None else [k[i].contiguous() for k in mask])
            out.append(h[-1])
        return out

    def forward_tick_rnn(self, score_tensor, beat_rnn_out, tick_seq_len, teacher_forced, sampling, mask=None, uniforms=None):
        if sampling not in ('argmax', 'multinomial'):
            raise NotImplementedError(f'sampling {sampling!r}: argmax and multinomial are implemented')
        b = score_tensor.size(0)
        if sampling == 'multinomial' and uniforms is None and not (self.use_teacher_forcing and teacher_forced):
            uniforms = self._sampling_uniforms(b, score_tensor.device)
        w_ih0, _, b_ih0, _ = self.rnn_tick.cell(0)
        prev = ops.broadcast_rows(self.x_0, b)                             # learned start embedding
        weights, samples = [], []
        for i, bo in enumerate(beat_rnn_out):
            h = self.hidden_init(bo, 'tick')                               # hidden is reset per beat
            beat_emb = _lin(bo, self.beat_emb_to_tick_rnn_input[0], ACT_SELU)
            for j in range(tick_seq_len):
                t = i * tick_seq_len + j
                inp = ops.concat_cols(prev, beat_emb)
                gi0 = ops.dense(inp, w_ih0, b_ih0, Link.dense(w_ih0.shape[1], w_ih0.shape[0]), ACT_NONE)
                h = self._stack_step(self.rnn_tick, gi0, h, None if mask is None else [k[t].contiguous() for k in mask])
                probs = _lin(h[-1], self.tick_emb_to_note_emb[0], ACT_RELU)
                if self.use_teacher_forcing and teacher_forced:
                    idx = score_tensor[:, t].contiguous()
                elif self._plan is not None and sampling == 'multinomial':
                    idx = ops.row_sample_planned(probs.detach(), uniforms[:, t].contiguous(), self._plan[2], t, self.temperature, *self._plan[:2])
                elif self._plan is not None:                   # the plan's argmax: top_k = 1, the draw without effect
                    idx = ops.row_sample_planned(probs.detach(), torch.ones(b, device=probs.device), self._plan[2], t, 1.0, 1, None)
                elif sampling == 'multinomial' and self._filter is not None:
                    idx = ops.row_sample_filtered(probs.detach(), uniforms[:, t].contiguous(), self.temperature, *self._filter)
                elif sampling == 'multinomial':
                    idx = ops.row_sample(probs.detach(), uniforms[:, t].contiguous(), self.temperature)
                else:
                    idx = ops.row_argmax(probs.detach())
                prev = ops.embed(idx.view(b, 1), self.note_embedding_layer.weight).view(b, -1)   # carries across beats
                weights.append(probs)
                samples.append(idx)
        return torch.stack(weights, 1), torch.stack(samples, 1)[:, None, :]


_PRIOR_CONSTANTS = {}


def _standard_normal_like(mu):
    """N(0, I) of mu's shape without a launch: loc / scale are expanded views of two cached device scalars (the reference
    fills two tensors per step: measure_vae.py:118-121); `_arvae_standard` lets compute_kld_loss use the closed form."""
    key = (mu.device, mu.dtype)
    if key not in _PRIOR_CONSTANTS:
        _PRIOR_CONSTANTS[key] = (torch.zeros((), device=mu.device, dtype=mu.dtype), torch.ones((), device=mu.device, dtype=mu.dtype))
    zero, one = _PRIOR_CONSTANTS[key]
    prior = distributions.Normal(loc=zero.expand(mu.shape), scale=one.expand(mu.shape), validate_args=False)
    prior._arvae_standard = True
    return prior


class MeasureVAE(Model):
    def __init__(self, dataset, note_embedding_dim=10, metadata_embedding_dim=2, num_encoder_layers=2,
                 encoder_hidden_size=512, encoder_dropout_prob=0.5, latent_space_dim=256, num_decoder_layers=2,
                 decoder_hidden_size=512, decoder_dropout_prob=0.5, has_metadata=True, dataset_type='folk'):
        super().__init__()
        self.dataset_type = dataset_type
        self.num_beats_per_measure, self.num_ticks_per_measure = 4, 24
        self.num_ticks_per_beat = 6
        self.dataset = repr(dataset)
        self.note_embedding_dim, self.metadata_embedding_dim = note_embedding_dim, metadata_embedding_dim
        self.num_encoder_layers, self.encoder_hidden_size = num_encoder_layers, encoder_hidden_size
        self.encoder_dropout_prob, self.latent_space_dim = encoder_dropout_prob, latent_space_dim
        self.num_decoder_layers, self.decoder_hidden_size = num_decoder_layers, decoder_hidden_size
        self.decoder_dropout_prob, self.has_metadata = decoder_dropout_prob, has_metadata
        self.num_notes = len(dataset.note2index_dicts)
        self.encoder = Encoder(note_embedding_dim, encoder_hidden_size, num_encoder_layers, self.num_notes,
                               encoder_dropout_prob, True, latent_space_dim, nn.GRU)
        self.decoder = HierarchicalDecoder(note_embedding_dim, self.num_notes, latent_space_dim, num_decoder_layers,
                                           decoder_hidden_size, decoder_dropout_prob, nn.GRU)
        self.update_filepath()

    def __repr__(self):
        return self.dataset_type + '_MeasureVAE' + self.trainer_config

    def arena_parameters(self):
        """every parameter once, in the order the trainer's flat arena should hold them: per encoder GRU layer the input
        projections of both directions side by side (weight_ih_l*, weight_ih_l*_reverse, then the two bias_ih), so that ONE
        whole-sequence GEMM applies both (Encoder._layer_sequence); everything else in module order.  state_dict keys and
        shapes are untouched (measurevae/encoder.py:27-34)."""
        gru = self.encoder.lstm
        first = []
        for layer in range(gru.num_layers):
            g = lambda n, suf: getattr(gru, f'{n}_l{layer}{suf}')
            first += [g('weight_ih', ''), g('weight_ih', '_reverse'), g('bias_ih', ''), g('bias_ih', '_reverse')]
        # the two heads' first layers read the same hidden vector; the tick RNN's initial state and its beat-embedding input are
        # two layers on the same beat output: each pair as one product (ops.dense_pair)
        enc, dec = self.encoder, self.decoder
        for la, lb in ((enc.linear_mean[0], enc.linear_log_std[0]), (dec.beat_emb_to_tick_rnn_hidden[0], dec.beat_emb_to_tick_rnn_input[0])):
            first += [la.weight, lb.weight, la.bias, lb.bias]
        taken = {id(p) for p in first}
        return first + [p for p in self.parameters() if id(p) not in taken]

    def push_noise(self, eps):
        self.encoder.push_noise(eps)

    def forward(self, measure_score_tensor, measure_metadata_tensor=None, train=True, *, need_prior_sample=True):
        """-> (weights, samples, z_dist, prior_dist, z_tilde, z_prior) as the reference (measure_vae.py:97-131).
        need_prior_sample=False (what this build's trainer passes: it never looks at z_prior, nor does the reference's):
        z_prior is None and the launch that would draw it is skipped."""
        if measure_score_tensor.size(1) != self.num_ticks_per_measure:
            raise AssertionError('a measure has 24 ticks')
        z_dist = self.encoder(measure_score_tensor)
        mu, z_tilde = z_dist.loc, z_dist._arvae_sample
        prior_dist = _standard_normal_like(mu)
        z_prior = ops.normal_noise(mu.shape, mu.device) if need_prior_sample else None     # the reference's second, unused draw
        weights, samples = self.decoder(z=z_tilde, score_tensor=measure_score_tensor, train=train)
        return weights, samples, z_dist, prior_dist, z_tilde, z_prior

    def forward_test(self, measure_score_tensor):
        """(B, M, 24) -> weights (B, M, 24, V), samples (B, 1, 24*M): every measure encoded, its code drawn, and decoded free-running
        with train=False, as the reference (measure_vae.py:133-166) -- there one encoder and one decoder call per measure, here ONE of
        each over the M*B rows in measure-major order (row = m*B + b), so that a pushed (M*B, Z) noise is the reference's draw order."""
        b, m, ticks = measure_score_tensor.shape
        if ticks != self.num_ticks_per_measure:
            raise AssertionError('a measure has 24 ticks')
        rows = measure_score_tensor.transpose(0, 1).reshape(m * b, ticks).contiguous()
        z_tilde = self.encoder(rows)._arvae_sample
        dummy = torch.zeros(m * b, ticks, dtype=torch.int64, device=rows.device)
        weights, samples = self.decoder(z=z_tilde, score_tensor=dummy, train=False)
        weights = weights.view(m, b, ticks, -1).transpose(0, 1).contiguous()
        samples = samples.view(m, b, ticks).transpose(0, 1).reshape(b, 1, m * ticks)
        return weights, samples

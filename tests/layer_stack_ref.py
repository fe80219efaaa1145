"""Float64 CPU restatement of MeasureVAE for any GRU layer count (test infrastructure for the --num_encoder_layers /
--num_decoder_layers tests; oracle/measure_vae.py is the two-layer one and stays so).

nn.GRU(num_layers=L): layer k > 0 reads layer k-1's outputs, dropout acts between layers only -- here an optional explicit
keep-mask per layer boundary (uint8, kept values scaled by 1 / (1 - p)):
    masks = {'enc': (Le-1, 24, B, 2H), 'beat': (Ld-1, 4, B, H), 'tick': (Ld-1, 24, B, H)}, time-major as the model's own.
  encoder : reference measurevae/encoder.py:27-51,94-124      decoder : measurevae/decoder.py:331-363,388-525
Checked against the reference's goldens in tests/test_measure_layers.py, which is what lets it stand in for the reference where the
goldens cannot: steps with dropout masks.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses
from oracle.image_vae import selu
from oracle.measure_vae import BEATS, TICKS, TICKS_PER_BEAT, gru_cell


def shapes(enc_layers, dec_layers, hid, v=35, emb=10, zdim=32):
    """state_dict key -> shape in the reference's registration order"""
    s = OrderedDict()
    g = 3 * hid
    for layer in range(enc_layers):
        for suf in ('', '_reverse'):
            s[f'encoder.lstm.weight_ih_l{layer}{suf}'] = (g, emb if layer == 0 else 2 * hid)
            s[f'encoder.lstm.weight_hh_l{layer}{suf}'] = (g, hid)
            s[f'encoder.lstm.bias_ih_l{layer}{suf}'] = (g,)
            s[f'encoder.lstm.bias_hh_l{layer}{suf}'] = (g,)
    s['encoder.note_embedding_layer.weight'] = (v, emb)
    for head in ('linear_mean', 'linear_log_std'):
        s[f'encoder.{head}.0.weight'] = (2 * hid, 2 * hid * enc_layers)
        s[f'encoder.{head}.0.bias'] = (2 * hid,)
        s[f'encoder.{head}.2.weight'] = (zdim, 2 * hid)
        s[f'encoder.{head}.2.bias'] = (zdim,)
    s['decoder.b_0'] = (1,)
    s['decoder.x_0'] = (emb,)
    s['decoder.note_embedding_layer.weight'] = (v, emb)
    s['decoder.z_to_beat_rnn_input.0.weight'] = (hid * dec_layers, zdim)
    s['decoder.z_to_beat_rnn_input.0.bias'] = (hid * dec_layers,)

    def gru(name, inp):
        for layer in range(dec_layers):
            s[f'decoder.{name}.weight_ih_l{layer}'] = (g, inp if layer == 0 else hid)
            s[f'decoder.{name}.weight_hh_l{layer}'] = (g, hid)
            s[f'decoder.{name}.bias_ih_l{layer}'] = (g,)
            s[f'decoder.{name}.bias_hh_l{layer}'] = (g,)
    gru('rnn_beat', 1)
    s['decoder.beat_emb_to_tick_rnn_hidden.0.weight'] = (hid * dec_layers, hid)
    s['decoder.beat_emb_to_tick_rnn_hidden.0.bias'] = (hid * dec_layers,)
    s['decoder.beat_emb_to_tick_rnn_input.0.weight'] = (hid, hid)
    s['decoder.beat_emb_to_tick_rnn_input.0.bias'] = (hid,)
    gru('rnn_tick', emb + hid)
    s['decoder.tick_emb_to_note_emb.0.weight'] = (v, hid)
    s['decoder.tick_emb_to_note_emb.0.bias'] = (v,)
    return s


def layer_counts(p):
    """(encoder layers, decoder layers) of a parameter dict"""
    return (sum(k.startswith('encoder.lstm.weight_hh_l') and not k.endswith('_reverse') for k in p),
            sum(k.startswith('decoder.rnn_tick.weight_hh_l') for k in p))


def _cell(p, prefix, x, h):
    return gru_cell(x, h, p[prefix.format('weight_ih')], p[prefix.format('weight_hh')], p[prefix.format('bias_ih')],
                    p[prefix.format('bias_hh')])


def _keep(h, mask, scale):
    return h if mask is None else h * mask.to(h.dtype) * scale


def encode(p, score, enc_masks=None, keep_scale=2.0):
    """score (B, 24) int64 -> (mu, log_std); enc_masks (L-1, 24, B, 2H) or None"""
    layers, _ = layer_counts(p)
    b = score.shape[0]
    hid = p['encoder.lstm.weight_hh_l0'].shape[1]
    seq = p['encoder.note_embedding_layer.weight'][score]                 # (B, 24, emb)
    finals = []
    for layer in range(layers):
        outs = []
        for suf in ('', '_reverse'):
            h = seq.new_zeros(b, hid)
            hs = [None] * TICKS
            for t in (range(TICKS) if suf == '' else range(TICKS - 1, -1, -1)):
                h = _cell(p, f'encoder.lstm.{{}}_l{layer}{suf}', seq[:, t], h)
                hs[t] = h
            finals.append(h)
            outs.append(torch.stack(hs, 1))
        seq = torch.cat(outs, 2)                                          # (B, 24, 2H)
        if layer < layers - 1 and enc_masks is not None:
            seq = _keep(seq, enc_masks[layer].transpose(0, 1), keep_scale)
    hcat = torch.cat(finals, 1)                                           # l0 fwd, l0 rev, l1 fwd, l1 rev, ...

    def head(name):
        t = selu(F.linear(hcat, p[f'encoder.{name}.0.weight'], p[f'encoder.{name}.0.bias']))
        return F.linear(t, p[f'encoder.{name}.2.weight'], p[f'encoder.{name}.2.bias'])
    return head('linear_mean'), head('linear_log_std')


def _stack_step(p, prefix, layers, x, h, masks, step, keep_scale):
    """one time step of an L-layer unidirectional stack; masks (L-1, T, B, H) or None -> the new states"""
    new = []
    for layer in range(layers):
        new.append(_cell(p, f'{prefix}.{{}}_l{layer}', x, h[layer]))
        if layer < layers - 1:
            x = _keep(new[-1], None if masks is None else masks[layer][step], keep_scale)
    return new


def decode(p, z, score, teacher_forced, beat_masks=None, tick_masks=None, keep_scale=2.0):
    """-> (weights (B, 24, V) >= 0, samples (B, 1, 24) int64); argmax with the lowest index on ties when not teacher-forced"""
    _, layers = layer_counts(p)
    b = z.shape[0]
    hid = p['decoder.rnn_beat.weight_hh_l0'].shape[1]

    def split(flat):                                                      # view(B, L, H).transpose(0, 1)
        return [flat[:, k * hid:(k + 1) * hid] for k in range(layers)]
    h = split(selu(F.linear(z, p['decoder.z_to_beat_rnn_input.0.weight'], p['decoder.z_to_beat_rnn_input.0.bias'])))
    b0 = p['decoder.b_0'].reshape(1, 1).expand(b, 1)
    beat_out = []
    for i in range(BEATS):
        h = _stack_step(p, 'decoder.rnn_beat', layers, b0, h, beat_masks, i, keep_scale)
        beat_out.append(h[-1])
    prev = p['decoder.x_0'].reshape(1, -1).expand(b, -1)
    weights, samples = [], []
    for i in range(BEATS):
        bo = beat_out[i]
        th = split(selu(F.linear(bo, p['decoder.beat_emb_to_tick_rnn_hidden.0.weight'], p['decoder.beat_emb_to_tick_rnn_hidden.0.bias'])))
        bemb = selu(F.linear(bo, p['decoder.beat_emb_to_tick_rnn_input.0.weight'], p['decoder.beat_emb_to_tick_rnn_input.0.bias']))
        for j in range(TICKS_PER_BEAT):
            t = i * TICKS_PER_BEAT + j
            th = _stack_step(p, 'decoder.rnn_tick', layers, torch.cat((prev, bemb), 1), th, tick_masks, t, keep_scale)
            probs = F.relu(F.linear(th[-1], p['decoder.tick_emb_to_note_emb.0.weight'], p['decoder.tick_emb_to_note_emb.0.bias']))
            idx = score[:, t] if teacher_forced else probs.detach().argmax(1)
            prev = p['decoder.note_embedding_layer.weight'][idx]
            weights.append(probs)
            samples.append(idx)
    return torch.stack(weights, 1), torch.stack(samples, 1)[:, None, :]


def step(state, score, eps, attr, reg_dims, beta, gamma, delta, teacher_forced, masks=None, keep_scale=2.0):
    """one loss evaluation and its gradients in float64: state {key: ndarray} -> dict(recons, dist, reg, loss, acc, z, mu, sigma,
    weights, samples, grads {key: ndarray})"""
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in state.items()}
    st = torch.from_numpy(np.ascontiguousarray(score))
    masks = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (masks or {}).items()}
    mu, log_std = encode(p, st, masks.get('enc'), keep_scale)
    sigma = torch.exp(log_std)
    z = mu + torch.from_numpy(np.ascontiguousarray(eps)).double() * sigma
    weights, samples = decode(p, z, st, teacher_forced, masks.get('beat'), masks.get('tick'), keep_scale)
    recons = losses.cross_entropy_mean(weights, st)
    dist = losses.kld_loss(mu, sigma, beta, 0.0)
    reg = losses.reg_loss(z, torch.from_numpy(np.ascontiguousarray(attr)).double(), reg_dims, gamma, delta) if len(reg_dims) else z.new_zeros(())
    loss = recons + dist + reg
    loss.backward()
    return dict(recons=float(recons.detach()), dist=float(dist.detach()), reg=float(reg.detach()), loss=float(loss.detach()),
                acc=float(losses.top1_accuracy(weights.detach(), st)),
                z=z.detach().numpy(), mu=mu.detach().numpy(), sigma=sigma.detach().numpy(), weights=weights.detach().numpy(),
                samples=samples.numpy(), grads={k: v.grad.numpy() for k, v in p.items()})

"""Goldens of the reference MeasureVAE at GRU layer counts other than two (--num_encoder_layers / --num_decoder_layers).

Run from a checkout that has the reference next to it (see make_goldens.py, whose stubs and helpers this imports):
    python tests/golden/make_layer_goldens.py
Writes
  measure_layers_e{E}d{D}_{mode}.npz   one MeasureVAETrainer step, the arrays of measure_step_*.npz (V = 35, z = 32, embedding 10,
                                       dropout 0, weight seed 4, logits spread as there)
  measure_layers_struct.json           per (E, D): the reference's state_dict keys and shapes in registration order and the repr
                                       strings of encoder, decoder and model
"""
import json
import os

import numpy as np
import torch

import make_goldens as mg
from make_goldens import EPS, MeasureVAE, MeasureVAETrainer, folk_dataset, grad_and_update_summaries, load_synth_weights, save, syn, t

# (encoder layers, decoder layers, hidden, batch, mode): mode tf / free = a training step with / without teacher forcing, eval = model.eval()
CASES = [(1, 1, 64, 20, 'tf'), (1, 1, 64, 20, 'free'), (3, 3, 64, 20, 'tf'), (3, 3, 64, 20, 'free'),
         (1, 3, 128, 21, 'free'), (3, 1, 128, 21, 'eval')]
STRUCT_CASES = [(1, 1), (2, 2), (3, 3), (4, 4), (1, 3), (3, 1)]
EPS_SEEDS = (41, 42, 43, 44)


def build(enc_layers, dec_layers, hidden):
    ds = folk_dataset()
    model = MeasureVAE(dataset=ds, note_embedding_dim=10, metadata_embedding_dim=2, num_encoder_layers=enc_layers,
                       encoder_hidden_size=hidden, encoder_dropout_prob=0.0, latent_space_dim=32, num_decoder_layers=dec_layers,
                       decoder_hidden_size=hidden, decoder_dropout_prob=0.0, has_metadata=False, dataset_type='folk')
    return ds, model


def layer_step(enc_layers, dec_layers, hidden, batch, mode, eseed):
    """make_goldens.measure_step at the given layer counts; None when the top-1 margin of this noise seed is too small"""
    ds, model = build(enc_layers, dec_layers, hidden)
    load_synth_weights(model, 4)
    with torch.no_grad():
        model.decoder.tick_emb_to_note_emb[0].bias.add_(0.5)
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(3.0)
    trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0, capacity=0.0,
                                rand=0, delta=10.0)
    train = mode != 'eval'
    model.train() if train else model.eval()
    model.decoder.teacher_forcing_prob = 1.0 if mode == 'tf' else 0.0
    score = t(syn.measure_batch(batch, seed=5 if train else 6))
    eps = syn.normal_noise((batch, 32), seed=eseed)
    before = {k: v.detach().numpy().copy() for k, v in model.named_parameters()}
    EPS.push(eps)
    weights, samples, z_dist, prior_dist, z_tilde, _ = model(score, score, train=train)
    recons = trainer.reconstruction_loss(x=score, x_recons=weights)
    dist_loss = trainer.compute_kld_loss(z_dist, prior_dist, trainer.beta)
    attr = trainer.compute_attribute_labels(score)
    reg = sum(trainer.compute_reg_loss(z_tilde, attr[:, d], d, gamma=trainer.gamma, factor=trainer.delta) for d in (0, 1, 2, 3))
    top2 = weights.detach().topk(2, dim=2)[0]
    margin = (top2[..., 0] - top2[..., 1]).min().item()
    if not margin > 1e-4:
        return None
    EPS.push(eps)
    trainer.zero_grad()
    loss, acc = trainer.loss_and_acc_for_batch((score, score), epoch_num=0, batch_num=0, train=train)
    loss.backward()
    trainer.step()
    assert abs(loss.item() - (recons + dist_loss + reg).item()) <= 1e-5 * abs(loss.item())
    wn = weights.detach().numpy()
    out = dict(recons=recons.item(), dist=dist_loss.item(), reg=reg.item(), loss=loss.item(), acc=acc.item(),
               z=z_tilde.detach().numpy(), mu=z_dist.loc.detach().numpy(), sigma=z_dist.scale.detach().numpy(),
               samples=samples.numpy(), attr=attr.numpy(), margin=margin, eseed=eseed,
               weights_sum=wn.astype(np.float64).sum(), weights_samp=wn.ravel()[syn.sample_indices('weights', wn.size, 128)],
               weights_row0=wn[0])
    out.update(grad_and_update_summaries(model, before))
    return out


def gen_steps():
    for enc_layers, dec_layers, hidden, batch, mode in CASES:
        for eseed in EPS_SEEDS:
            out = layer_step(enc_layers, dec_layers, hidden, batch, mode, eseed)
            if out is not None:
                break
        assert out is not None, f'no noise seed of {EPS_SEEDS} gives a top-1 margin > 1e-4'
        assert out['margin'] > 1e-4
        save(f'measure_layers_e{enc_layers}d{dec_layers}_{mode}.npz', **out)


def gen_struct():
    struct = {}
    for enc_layers, dec_layers in STRUCT_CASES:
        _, model = build(enc_layers, dec_layers, 64)
        struct[f'e{enc_layers}d{dec_layers}'] = dict(
            keys=[[k, list(v.shape)] for k, v in model.state_dict().items()],
            encoder_repr=repr(model.encoder), decoder_repr=repr(model.decoder), model_repr=repr(model))
    path = os.path.join(mg.HERE, 'measure_layers_struct.json')
    with open(path, 'w') as f:
        json.dump(struct, f, indent=1)
    print(f'wrote measure_layers_struct.json: {os.path.getsize(path) / 1024:.1f} KB')


if __name__ == '__main__':
    gen_steps()
    gen_struct()

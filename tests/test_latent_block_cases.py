"""CPU checks of what the latent block's float64 bars stand on (latent_block_cases.py): the restatement is the oracle's model and
loss, the screened batches have no unit near a gate, the fp32 CPU yardstick is then free of flips and small, and the bar
e <= R * e_cpu + FLOOR catches a member workgroup's slice of one product going missing for the rows of the last cluster only.

Figures these tests print (torch on 8 CPU threads; they move a little with the thread count, as the fp32 kernels' blocking does):
  kind      B    width  pool  yardstick  tau       pass rate  flips  largest gradient e_cpu
  dsprites  1    -      6     2.2e-06    3.5e-05   0.83       0      1.2e-06
  dsprites  33   -      198   8.1e-06    1.3e-04   0.49       0      9.5e-07
  dsprites  72   -      432   1.0e-05    1.6e-04   0.40       0      7.3e-07
  dsprites  259  -      1554  9.8e-06    1.6e-04   0.42       0      1.0e-06
  dsprites  515  -      3090  1.2e-05    1.9e-04   0.33       0      1.3e-06
  mnist     1    256    6     1.1e-06    1.8e-05   0.83       0      6.6e-07
  mnist     3    256    18    2.3e-06    3.6e-05   0.83       0      6.9e-07
  mnist     47   256    282   3.4e-06    5.4e-05   0.80       0      4.6e-07
  mnist     67   256    402   3.9e-06    6.3e-05   0.79       0      5.7e-07
  mnist     5    40     30    1.5e-06    2.4e-05   0.87       0      5.4e-07
  mnist     5    52     30    1.6e-06    2.5e-05   0.93       0      4.7e-07
  mnist     5    32     30    1.7e-06    2.6e-05   0.90       0      5.8e-07
  mnist     5    64     30    1.6e-06    2.5e-05   1.00       0      5.9e-07
The yardstick is a maximum over the pool and one row can carry it: with the weights of seed 7 and the dSprites pool of seed 3001 a
single row (a large sigma times a large eps) puts it at 3.3e-05, tau at 5.3e-04 and the pass rate at 0.06, under the 1 / 6 a pool of
six batches needs; the other rows' median is 2e-06.  The cases use weight seed 9, where no pool has such a row.
"""
import numpy as np
import pytest
import torch

import latent_block_cases as lbc
from latent_block_cases import FLOOR, R
from oracle import image_vae as o_vae
from oracle import losses as o_losses


ALL_CASES = [c + (None,) for c in lbc.CASES] + lbc.WIDTH_CASES


@pytest.mark.parametrize('kind,batch,width', ALL_CASES, ids=[f'{k}_b{b}' + (f'_w{w}' if w else '') for k, b, w in ALL_CASES])
def test_screened_batch_has_no_unit_near_a_gate_and_a_quiet_yardstick(kind, batch, width):
    c = lbc.case(kind, batch, width)
    ref, cpu = c['ref'], c['cpu']
    assert c['x'].shape[0] == batch and c['passed'] >= batch and c['tau'] == lbc.TAU_FACTOR * c['yardstick']
    # on the kept rows every ReLU / SELU unit is at least tau * rms(layer) from zero in float64 ...
    margin = min(float(np.abs(v).min()) / c['rms'][k] for k, v in ref['pre'].items())
    units = sum(v[0].size for v in ref['pre'].values())
    assert margin >= c['tau'], (margin, c['tau'])
    # ... so the fp32 CPU yardstick takes every gate the way float64 does
    n_flips = lbc.flips(ref, cpu)
    assert n_flips == 0
    worst = 0.0
    for name, g in ref['grads'].items():
        assert np.any(g != 0), name
        e = lbc.rel(cpu['grads'][name], g)
        worst = max(worst, e)
        assert e <= lbc.E_CPU_CEILING, (name, e)
    e_logits = lbc.rel(cpu['logits'], ref['logits'])
    rms_logits = float(np.sqrt(np.mean(ref['logits'] ** 2)))
    print(f'{kind} B={batch}: {units} screened units per row, smallest |pre| / rms {margin:.3e} (tau {c["tau"]:.3e}), flips {n_flips}, '
          f'largest gradient e_cpu {worst:.3e}, logits e_cpu {e_logits:.3e}, logits rms {rms_logits:.3f}')
    if kind == 'mnist':
        assert 0.02 <= rms_logits <= 8.0, rms_logits       # else: another gain (latent_block_cases.GAIN), not another test


@pytest.mark.parametrize('kind,batch', [('dsprites', 5), ('mnist', 3)])
def test_restatement_is_the_oracle(kind, batch):
    """regime 'full', float32: oracle.image_vae.forward bit for bit.  Block regimes, float64: the hand-written gradients equal
    torch autograd of the oracle's loss formulas on the same forward pass, relative L2 1e-12."""
    state = lbc.syn.synth_state(o_vae.SHAPES[kind], 3, lbc.GAIN[kind])
    x, lab, eps, masks = lbc.inputs(kind, batch, 77)
    p, xt, lt, et, mt = lbc._tensors(state, x, lab, eps, masks, torch.float32)
    with torch.no_grad():
        mine = lbc.forward(kind, 'full', p, xt, et, mt)
        logits, mu, sigma, z = o_vae.forward(kind, p, xt, et, mt)
    for a, b in ((mine['logits'], logits), (mine['mu'], mu), (mine['sigma'], sigma), (mine['z'], z)):
        assert torch.equal(a, b)
    regime = lbc.REGIME_OF[kind]
    got = lbc.step(kind, regime, state, x, lab, eps, masks, torch.float64)
    p, xt, lt, et, mt = lbc._tensors(state, x, lab, eps, masks, torch.float64)
    for v in p.values():
        v.requires_grad_(True)
    fw = lbc.forward(kind, regime, p, xt, et, mt)
    recon = o_losses.bce_with_logits_per_batch(fw['logits'], xt)
    dist = o_losses.kld_loss(fw['mu'], fw['sigma'], lbc.BETA, lbc.CAPACITY)
    reg = o_losses.reg_loss(fw['z'], lt, lbc.REG_DIMS[kind], lbc.GAMMA, lbc.DELTA)
    (recon + dist + reg).backward()
    s = got['scalars']
    for mine_s, want in ((s['recon'], recon), (s['dist'], dist), (s['reg'], reg), (s['loss'], recon + dist + reg)):
        assert abs(mine_s - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    assert abs(s['acc'] - float(o_losses.pixel_accuracy(fw['logits'].detach(), xt))) <= 2.0 ** -23      # (the oracle's mean is an fp32 one)
    assert set(got['grads']) == set(state)
    for name, v in p.items():
        assert lbc.rel(got['grads'][name], v.grad.numpy()) <= 1e-12, name


@pytest.mark.parametrize('batch', [33, 259])
def test_the_bar_catches_a_dropped_slice_in_the_last_cluster(batch):
    """The separation the GPU bars rely on: the fp32 restatement with one 16-column slice of enc_lin.2's product missing for the
    rows of the last cluster only (B = 33: one row of 33; B = 259: three rows of 259) must break e <= R * e_cpu + FLOOR on mu, z or
    a gradient tensor.  Prints every tensor that breaks.  At both batches all 34 do -- mu, sigma, z, the logits and every parameter's
    gradient: mu by 4.8e-02 (B = 33) and 2.8e-02 (B = 259) against bars of 2.9e-06, the least affected one, dec_conv.6.bias at
    B = 259, by 1.8e-06 against 2.2e-07."""
    c = lbc.case('dsprites', batch)
    bad = lbc.step('dsprites', c['regime'], c['state'], c['x'], c['labels'], c['eps'], c['masks'], torch.float32,
                   mutate=lbc.drop_slice_mutation(batch, c['state']['enc_lin.2.bias']))
    ref, cpu = c['ref'], c['cpu']
    broken = []
    for name in ('mu', 'sigma', 'z', 'logits'):
        e, e_cpu = lbc.rel(bad[name], ref[name]), lbc.rel(cpu[name], ref[name])
        if not e <= R * e_cpu + FLOOR:
            broken.append((name, e, e_cpu))
    for name in ref['grads']:
        e, e_cpu = lbc.rel(bad['grads'][name], ref['grads'][name]), lbc.rel(cpu['grads'][name], ref['grads'][name])
        if not e <= R * e_cpu + FLOOR:
            broken.append((name, e, e_cpu))
    for name, e, e_cpu in broken:
        print(f'B={batch} dropped slice breaks {name}: e {e:.3e}  e_cpu {e_cpu:.3e}  bar {R * e_cpu + FLOOR:.3e}')
    names = {n for n, _, _ in broken}
    assert names & ({'mu', 'z'} | set(ref['grads'])), 'the bar does not see the fault'

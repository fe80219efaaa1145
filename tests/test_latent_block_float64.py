"""The latent block -- the Linear stack, the two heads and the reparameterisation as ONE launch per pass -- against float64, per
tensor: the clustered pair of csrc/midcluster.hip (with the two folded 8x8 <-> 4x4 conv layers of the dSprites model), the row
kernels of csrc/midblock.hip at one, two and four rows per workgroup, and the row kernel between the wide tile GEMMs of the
Morpho-MNIST model.  Needs a real MI355X.

The block is reachable only through arvae_image_vae_forward / _backward, so every case is one whole forward + backward of the
trainer on a SCREENED batch in a regime that keeps the activations where the block needs them (latent_block_cases.py: why, and
what test_latent_block_cases.py proves about it on the CPU).  Compared one by one: mu, sigma, z, the logits and every parameter's
gradient, sliced from the optimizer's gradient arena by its offsets.

Bar (split_cases.py):  e_hip <= R * e_cpu + FLOOR,  R = 4, FLOOR = 1e-7, e_* the relative L2 distance to float64 of the HIP result / of
the fp32 CPU restatement.  Scalars (loss, recon, dist, reg, KL):  |s_hip - s64| <= R |s32 - s64| + FLOOR |s64|.  Accuracy: every pixel
whose |logit64| exceeds 16 x the yardstick's largest absolute logit error has the float64 sign in the HIP logits, and the accuracy
scalar equals the mean computed from the HIP logits to 2^-23 relative (a count that fp32 holds exactly times a rounded 1 / N:
two roundings of 2^-24 each).  The tensors are listed in dependency order -- mu, sigma, z, logits, then the gradients from the
decoder back -- so the first one reported over the bar is where a fault starts.

Which kernels ran is read from the launch record (arvae_profile_begin / _end: one line per check_launch() label).

Not barred here (the float64 reference is the cost: Morpho-MNIST above ~70 rows takes tens of seconds): the Morpho-MNIST model at
two and four rows per workgroup (B > 256), and any batch above 1024, where the workgroups' AMAX units no longer fit the array
(AMAX_N) and the maximum moves to a launch of its own.  The whole-step tests of test_hip_parity.py cover those at 2e-3.
"""
import ctypes

import numpy as np
import pytest
import torch

import latent_block_cases as lbc
from latent_block_cases import FLOOR, R

pytestmark = pytest.mark.gpu

SCALARS = ('loss', 'recon', 'dist', 'reg', 'kl')
CLUSTER_FWD, CLUSTER_BWD = 'midc_forward_kernel(+ conv4, deconv1)', 'midc_backward_kernel(+ conv4, deconv1)'
ROWS_FWD, ROWS_BWD = 'mid_forward_kernel', 'mid_backward_kernel'
WIDE = ('wide_gemm(partial)', 'wide_gemm(full)', 'wide_wgrad')


class DspritesDataset:
    pass


class MorphoMnistDataset:
    pass


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


def _model(kind, width=None):
    from arvae_amd import image_vae as iv
    if kind == 'dsprites':
        return iv.DspritesVAE()
    m = iv.MnistVAE()
    if width is not None:       # the Morpho-MNIST-shaped model with another hidden width (test_hip_parity.py, the LDS growth test)
        m.enc_lin = iv.LayerStack([(0, iv._dense(2888, width))])
        m.enc_mean, m.enc_log_std = iv._dense(width, 16), iv._dense(width, 16)
        m.dec_lin = iv.LayerStack([(0, iv._dense(16, width)), (2, iv._dense(width, 2888))])
        m.enc_lin_plan = [(0, iv.Link.dense(2888, width, in_perm=(8, 361)))]
        m.dec_lin_plan = [(0, iv.Link.dense(16, width)), (2, iv.Link.dense(width, 2888, out_perm=(8, 361)))]
        m.head_link = iv.Link.dense(width, 16)
    return m


def _trainer(kind, state, no_cluster=False, width=None):
    """the trainer of test_clustered_latent_block_handoffs_under_load with the regime's activations written into the executor's
    (cached) descriptor before the first pass; -> (trainer, model, {'scalars': the pass's scalar block})"""
    from arvae_amd import ops
    from arvae_amd.fused import FusedImageVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    model = _model(kind, width)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    ds = DspritesDataset() if kind == 'dsprites' else MorphoMnistDataset()
    trainer = ImageVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=lbc.REG_DIMS[kind], dec_dist='bernoulli', beta=lbc.BETA,
                              gamma=lbc.GAMMA, capacity=lbc.CAPACITY, rand=0, delta=lbc.DELTA)
    trainer.cuda()
    model.train()
    fused = trainer._fused = FusedImageVAE(model, trainer.optimizer, trainer.reg_dim, trainer.beta, trainer.gamma, trainer.delta,
                                           trainer.dec_dist)
    fused.no_cluster = bool(no_cluster)
    d = fused.descriptor()
    code = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'selu': ops.ACT_SELU}
    a_enc, a_dec = lbc.acts(kind, lbc.REGIME_OF[kind])
    assert d.n_enc == len(a_enc) and d.n_dec == len(a_dec)
    for i, a in enumerate(a_enc):
        d.enc[i].act = code[a]
    for i, a in enumerate(a_dec):
        d.dec[i].act = code[a]
    seen = {}
    run = fused.run

    def recording_run(*args, **kw):
        out = run(*args, **kw)
        seen['scalars'] = out[1]
        return out
    fused.run = recording_run
    return trainer, model, seen


def _pass(trainer, model, seen, c, dev):
    """one forward + backward on the case's batch -> dict(tensors {name: array} in dependency order, scalars, acc, labels (the
    launch record's names))"""
    from arvae_amd import _lib
    from arvae_amd.fused import ACC, DIST, KL, LOSS, RECON, REG
    lib = _lib.load()
    xt, lt = torch.from_numpy(c['x']).to(dev), torch.from_numpy(c['labels']).to(dev)
    model.push_noise(torch.from_numpy(c['eps']))
    if c['masks'] is not None:
        model.push_dropout_masks([torch.from_numpy(m).permute(0, 2, 3, 1).contiguous() for m in c['masks']])
    trainer.zero_grad()
    torch.cuda.synchronize()
    lib.arvae_profile_begin(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    try:
        loss, _acc = trainer.loss_and_acc_for_batch((xt, lt), 0, 0, True)
        loss.backward()
    finally:
        buf = ctypes.create_string_buffer(1 << 16)
        lib.arvae_profile_end(buf, len(buf))
    torch.cuda.synchronize()
    labels = [ln.split('\t')[0] for ln in buf.value.decode().splitlines()]
    s = seen['scalars'].detach().cpu().numpy().astype(np.float64)             # read after backward: the finishing step may be deferred
    outs = trainer.last_outputs
    tensors = {k: outs[k].detach().cpu().numpy() for k in ('mu', 'sigma', 'z', 'logits')}
    opt = trainer.optimizer
    arena = opt.grad_arena.detach().cpu().numpy()
    name_of = {id(p): k for k, p in model.named_parameters()}
    by_name = {name_of[id(p)]: arena[off:off + p.numel()].reshape(tuple(p.shape)).copy() for p, off in zip(opt.params, opt._offsets)}
    for name in c['ref']['grads']:                                             # (the reference's order: from the decoder back)
        tensors[name] = by_name[name]
    assert set(by_name) == set(c['ref']['grads'])
    return dict(tensors=tensors, labels=labels, acc=float(s[ACC]),
                scalars=dict(loss=s[LOSS], recon=s[RECON], dist=s[DIST], reg=s[REG], kl=s[KL]))


def _flat(step_result):
    t = {k: step_result[k] for k in ('mu', 'sigma', 'z', 'logits')}
    t.update(step_result['grads'])
    return t


def _hold(case, got, c):
    """the bar on every tensor of one pass (module docstring); prints e_hip / e_cpu per tensor"""
    ref, cpu = _flat(c['ref']), _flat(c['cpu'])
    bad = []
    for k, g in got['tensors'].items():
        assert np.all(np.isfinite(g)), (case, k)
        e_hip, e_cpu = lbc.rel(g.reshape(ref[k].shape), ref[k]), lbc.rel(cpu[k], ref[k])
        ratio = e_hip / e_cpu if e_cpu > 0 else float('inf' if e_hip > 0 else 0)
        print(f'{case} {k}: e_hip {e_hip:.3e}  e_cpu {e_cpu:.3e}  e_hip/e_cpu {ratio:.2f}  bar {R * e_cpu + FLOOR:.3e}')
        if not e_hip <= R * e_cpu + FLOOR:
            bad.append((k, e_hip, e_cpu))
    assert not bad, (case, 'first over the bar: ' + str(bad[0][0]), bad)


def _hold_scalars(case, got, c):
    """the scalars' bar and the two accuracy checks of one pass (module docstring)"""
    bad = []
    for k in SCALARS:
        s_hip, s64, s32 = float(got['scalars'][k]), c['ref']['scalars'][k], c['cpu']['scalars'][k]
        bar = R * abs(s32 - s64) + FLOOR * abs(s64)
        print(f'{case} {k}: hip {s_hip:.9g}  float64 {s64:.9g}  |hip - f64| {abs(s_hip - s64):.3e}  |cpu - f64| {abs(s32 - s64):.3e}  bar {bar:.3e}')
        if not abs(s_hip - s64) <= bar:
            bad.append((k, abs(s_hip - s64), abs(s32 - s64)))
    # what the KL kernel adds to the error of its inputs: the KL mean of the HIP mu and sigma, evaluated in float64
    mu, sigma = (got['tensors'][k].astype(np.float64) for k in ('mu', 'sigma'))
    kl_in = float((0.5 * (sigma * sigma + mu * mu - 1.0 - np.log(sigma * sigma))).sum(1).mean())
    print(f'{case} kl: float64 KL of the HIP mu, sigma {kl_in:.9g}  |hip - that| {abs(float(got["scalars"]["kl"]) - kl_in):.3e} '
          f'(one fp32 rounding of it: {2.0 ** -24 * kl_in:.3e})')
    # accuracy: the float64 side of every pixel that is clear of zero, and the scalar against the HIP logits themselves
    l_hip, l64 = got['tensors']['logits'].reshape(c['ref']['logits'].shape).astype(np.float64), c['ref']['logits']
    clear = np.abs(l64) > 16.0 * np.abs(c['cpu']['logits'] - l64).max()
    wrong = int(((l_hip >= 0) != (l64 >= 0))[clear].sum())
    mean = float(((l_hip >= 0) == (c['x'].reshape(l64.shape) >= 0.5)).mean())
    print(f'{case} acc: hip {got["acc"]:.9g}  from the HIP logits {mean:.9g}  pixels clear of zero {int(clear.sum())} of {clear.size}, wrong side {wrong}')
    if wrong:
        bad.append(('logit signs', wrong, 0))
    if not abs(got['acc'] - mean) <= 2.0 ** -23 * mean:
        bad.append(('acc', got['acc'], mean))
    assert not bad, (case, 'first over the bar: ' + str(bad[0][0]), bad)


def _assert_path(path, labels):
    if path == 'cluster':
        assert CLUSTER_FWD in labels and CLUSTER_BWD in labels, labels
        assert ROWS_FWD not in labels and ROWS_BWD not in labels, labels
    else:
        assert ROWS_FWD in labels and ROWS_BWD in labels, labels
        assert not [n for n in labels if n.startswith('midc_')], labels
    if path == 'wide':
        assert all(n in labels for n in WIDE), labels
    elif path != 'cluster':
        assert not [n for n in labels if n.startswith('wide_')], labels


def _assert_clean(trainer):
    """no hand-off gave up: the status word is zero and the trainer has not left the clustered kernels"""
    assert int(trainer.optimizer.status_words()[0].item()) == 0
    assert trainer._fused.no_cluster is False


_RESULTS = {}


def _case_of(path, batch, width=None):
    return lbc.case('mnist' if (path == 'wide' or width is not None) else 'dsprites', batch, width)


def _warm_passes(dev):
    """two passes of ONE trainer on the clustered kernels, B = 33 and then B = 72"""
    first, second = _case_of('warm1', 33), _case_of('warm2', 72)
    trainer, model, seen = _trainer('dsprites', first['state'])
    for key, c in ((('warm1', 33, None), first), (('warm2', 72, None), second)):
        _RESULTS[key] = _pass(trainer, model, seen, c, dev)
        _assert_clean(trainer)


def _result(path, batch, dev, width=None):
    """the pass of (path, batch, width) on a fresh trainer (the warm pair: on one), run once per module"""
    key = (path, batch, width)
    if key not in _RESULTS:
        if path.startswith('warm'):
            _warm_passes(dev)
            return _RESULTS[key]
        c = _case_of(path, batch, width)
        trainer, model, seen = _trainer('mnist' if (path == 'wide' or width is not None) else 'dsprites', c['state'],
                                        no_cluster=(path == 'rows'), width=width)
        got = _pass(trainer, model, seen, c, dev)
        if path == 'cluster':
            _assert_clean(trainer)
        _RESULTS[key] = got
    return _RESULTS[key]


@pytest.mark.parametrize('batch', lbc.CLUSTER_BATCHES)
def test_clustered_pair_vs_float64(dev, batch):
    """midc_forward_kernel / midc_backward_kernel with the folded conv layers: one cluster with one valid row; a second cluster
    with one row; three clusters (no multiple of the 8 XCDs), the last with 8 rows; nine clusters, the last with 3 rows"""
    got = _result('cluster', batch, dev)
    _assert_path('cluster', got['labels'])
    _hold(f'cluster B={batch}', got, lbc.case('dsprites', batch))


@pytest.mark.parametrize('batch', lbc.ROWS_BATCHES)
def test_row_kernels_vs_float64(dev, batch):
    """mid_forward_kernel<R> / mid_backward_kernel<R> on the dSprites block (no_cluster): R = 1 (B = 1, 33), R = 2 with a last
    workgroup of one row (B = 259), R = 4 with a last workgroup of three (B = 515)"""
    got = _result('rows', batch, dev)
    _assert_path('rows', got['labels'])
    _hold(f'rows B={batch}', got, lbc.case('dsprites', batch))


@pytest.mark.parametrize('batch', lbc.MNIST_BATCHES)
def test_row_kernel_between_the_wide_gemms_vs_float64(dev, batch):
    """Morpho-MNIST: the 2888-wide layers on the 64 x 64 tile GEMMs (split reduction finished in the row kernel's prologue, SELU and
    the keep-mask of enc_conv.6 applied by the wide data-gradient GEMM), everything between them in the row kernel; train mode"""
    got = _result('wide', batch, dev)
    _assert_path('wide', got['labels'])
    _hold(f'mnist B={batch}', got, lbc.case('mnist', batch))


@pytest.mark.parametrize('batch', [33, 259])
def test_clustered_and_row_kernels_are_two_paths(dev, batch):
    """Both within the bar (the two tests above) and NOT bit-identical in at least one gradient tensor: they sum in different orders.
    Bit-identical results mean the switch between the paths did not take."""
    a, b = _result('cluster', batch, dev), _result('rows', batch, dev)
    _assert_path('cluster', a['labels'])
    _assert_path('rows', b['labels'])
    c = lbc.case('dsprites', batch)
    differ = [k for k in c['ref']['grads'] if not np.array_equal(a['tensors'][k], b['tensors'][k])]
    print(f'B={batch}: {len(differ)} of {len(c["ref"]["grads"])} gradient tensors differ in at least one bit between the two paths')
    assert differ


def test_clustered_pair_on_a_warm_workspace(dev):
    """A second pass of the SAME trainer at another batch (33, then 72): prepared matrices, arrival counters and ticket heads are
    what the first pass left.  Both passes meet the bar."""
    for path, batch in (('warm1', 33), ('warm2', 72)):
        got = _result(path, batch, dev)
        _assert_path('cluster', got['labels'])
        _hold(f'{path} B={batch}', got, _case_of(path, batch))


def _width_path(width):
    return 'rows' if width % 32 else 'wide'


@pytest.mark.parametrize('width', [w for _, _, w in lbc.WIDTH_CASES])
def test_narrow_hidden_widths_vs_float64(dev, width):
    """The Morpho-MNIST-shaped model at hidden widths 40 and 52, B = 5: neither is a multiple of the tile GEMMs' 32-wide reduction
    chunk, so the 2888-wide layers have to stay on the row kernels.  At 40 the planes' padding already kept them there (they do not
    fit the fp32 layouts' space); at 52 mid_describe() used to hand them to the tile GEMMs, whose precondition then stopped the pass
    with ARVAE_E_INVALID ("does not fit the tile GEMM"), and now checks that precondition first.  Widths 32 and 64 stay on the tile
    GEMMs.  All four through the same bar."""
    got = _result(_width_path(width), 5, dev, width)
    _assert_path(_width_path(width), got['labels'])
    _hold(f'mnist width {width} B=5', got, _case_of('wide', 5, width))


SCALAR_PASSES = [('cluster', b, None) for b in lbc.CLUSTER_BATCHES] + [('rows', b, None) for b in lbc.ROWS_BATCHES] + \
                [('wide', b, None) for b in lbc.MNIST_BATCHES] + [('warm1', 33, None), ('warm2', 72, None)] + \
                [(_width_path(w), 5, w) for _, _, w in lbc.WIDTH_CASES]


@pytest.mark.parametrize('path,batch,width', SCALAR_PASSES, ids=[f'{p}_b{b}' + (f'_w{w}' if w else '') for p, b, w in SCALAR_PASSES])
def test_scalars_and_accuracy_vs_float64(dev, path, batch, width):
    """loss, recon, dist, reg, KL and the accuracy of every pass above (the passes themselves are not run again).

    What this test found: with the KL elements 0.5 (sigma^2 + mu^2 - 1 - log sigma^2) evaluated and summed in fp32 (where sigma is
    near 1 the last three terms cancel to a few ulp of 1) the KL mean sat 0.6 - 1.1 ulp from the float64 KL of the kernel's OWN mu
    and sigma (the "float64 KL of the HIP mu, sigma" line), and at mnist B = 1 and 3 that put KL and dist = 4 KL over the bar:
    |hip - f64| 2.63e-07 against 2.28e-07 and 4.14e-07 against 4.02e-07.  The finishing step (csrc/vae_finish.h) and kld_fwd_kernel
    now evaluate and sum the elements in double, so the KL mean is the correctly rounded mean of its inputs."""
    _hold_scalars(f'{path} B={batch}' + (f' width {width}' if width else ''), _result(path, batch, dev, width), _case_of(path, batch, width))

"""The digit classifier on the GPU: every convolution geometry, the stem, the epilogue, the pool and the whole network against
float64 (bar of tests/split_cases.py: e_hip <= R e_cpu + FLOOR, R = 4, FLOOR = 1e-7), the weight preparation's invalidation,
ImageVAETrainer.get_resnet_accuracy against what it classified, and the CLI.  The fixture is tests/resnet_ref.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import arvae_amd  # noqa: E402,F401
import resnet_ref  # noqa: E402
from split_cases import FLOOR, R  # noqa: E402
from test_data_gpu import write_mnist  # noqa: E402

pytestmark = pytest.mark.gpu
BATCHES = (1, 3, 67)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def fixture():
    return resnet_ref.Fixture(67)


@pytest.fixture(scope='module')
def model(fixture, dev):
    from arvae_amd.mnist_resnet import MnistResNet
    m = MnistResNet()
    m.load_state_dict(fixture.sd)
    return m.to(dev).eval()


def nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


def bar(name, got, want64, cpu32):
    e_hip, e_cpu = resnet_ref.rel_l2(got, want64), resnet_ref.rel_l2(cpu32, want64)
    print(f'{name}: e_hip {e_hip:.3e}  e_cpu {e_cpu:.3e}  ratio {e_hip / max(e_cpu, 1e-30):.2f}')
    assert e_hip <= R * e_cpu + FLOOR, (name, e_hip, e_cpu)
    return e_hip, e_cpu


# ---- 1. one convolution at a time ---------------------------------------------------------------------------------------
# (input side, C_in, C_out, kernel, stride): every distinct geometry of the net
CONV_CASES = {'c64_7': (7, 64, 64, 3, 1), 'c64to128_7s2': (7, 64, 128, 3, 2), 'd64to128_7s2': (7, 64, 128, 1, 2),
              'c128_4': (4, 128, 128, 3, 1), 'c128to256_4s2': (4, 128, 256, 3, 2), 'c256_2': (2, 256, 256, 3, 1),
              'c256to512_2s2': (2, 256, 512, 3, 2), 'c512_1': (1, 512, 512, 3, 1)}


@pytest.mark.parametrize('name', list(CONV_CASES))
def test_convolution_against_float64(dev, name):
    from arvae_amd import ops
    hin, cin, cout, k, stride = CONV_CASES[name]
    g = ops.ResnetConv(hin, cin, cout, k, stride)
    rs = np.random.RandomState(len(name) * 131 + hin)
    w = torch.from_numpy(rs.normal(0, np.sqrt(2.0 / (cout * k * k)), (cout, cin, k, k)).astype(np.float32))
    prep = ops.resnet18_conv_prepare(g, w.to(dev))                 # no BN: w' = w, zero bias; the map is linear
    x_all = torch.from_numpy(rs.normal(0, 1, (max(BATCHES), cin, hin, hin)).astype(np.float32))
    for n in BATCHES:
        x = x_all[:n]
        got = nchw(ops.resnet18_conv(g, prep, nhwc(x, dev)))
        want = F.conv2d(x.double(), w.double(), None, stride, g.pad)
        assert tuple(got.shape) == tuple(want.shape) == (n, cout, g.hout, g.hout)
        bar(f'{name} n={n} (M={n * g.hout ** 2}, K={len(ops.resnet18_live_taps(g)) * cin})', got, want, F.conv2d(x, w, None, stride, g.pad))


def test_stem_against_float64(dev):
    from arvae_amd import ops
    rs = np.random.RandomState(77)
    w = torch.from_numpy(rs.normal(0, np.sqrt(2.0 / (64 * 49)), (64, 1, 7, 7)).astype(np.float32))
    prep = ops.resnet18_stem_prepare(w.to(dev))
    x_all = torch.from_numpy(resnet_ref.stroke_images(max(BATCHES), 5) + rs.normal(0, 0.05, (max(BATCHES), 1, 28, 28)).astype(np.float32))
    for n in BATCHES:
        x = x_all[:n].contiguous()
        got = nchw(ops.resnet18_stem(prep, x.to(dev), relu=False))
        bar(f'stem n={n}', got, F.conv2d(x.double(), w.double(), None, 2, 3), F.conv2d(x, w, None, 2, 3))


# ---- 2. epilogue and pool -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c64_7', 'c64to128_7s2', 'c256to512_2s2'])
def test_epilogue_is_exact(dev, name):
    """the same prepared weights with and without a bias: + b', + residual, ReLU, in that order, each one fp32 rounding"""
    from arvae_amd import ops
    hin, cin, cout, k, stride = CONV_CASES[name]
    g = ops.ResnetConv(hin, cin, cout, k, stride)
    rs = np.random.RandomState(9)
    n = 5
    w = torch.from_numpy(rs.normal(0, np.sqrt(2.0 / (cout * k * k)), (cout, cin, k, k)).astype(np.float32)).to(dev)
    gamma, var = (torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32)).to(dev) for _ in range(2))
    beta, mean = (torch.from_numpy(rs.normal(0, 0.2, cout).astype(np.float32)).to(dev) for _ in range(2))
    zero = torch.zeros(cout, device=dev)
    plain = ops.resnet18_conv_prepare(g, w, (gamma, zero, zero, var))             # same scale, b' = 0
    biased = ops.resnet18_conv_prepare(g, w, (gamma, beta, mean, var))
    assert torch.equal(plain[:-cout], biased[:-cout]) and torch.equal(plain[-cout:], zero)
    b = biased[-cout:]
    want_b = (beta.double() - mean.double() * gamma.double() / torch.sqrt(var.double() + 1e-5)).float()
    assert float((b - want_b).abs().max()) <= 2.0 ** -23 * float(want_b.abs().max())
    x = torch.from_numpy(rs.normal(0, 1, (n, hin, hin, cin)).astype(np.float32)).to(dev)
    res = torch.from_numpy(rs.normal(0, 1, (n, g.hout, g.hout, cout)).astype(np.float32)).to(dev)
    product = ops.resnet18_conv(g, plain, x)
    assert torch.equal(ops.resnet18_conv(g, biased, x), product + b)
    assert torch.equal(ops.resnet18_conv(g, biased, x, relu=True), torch.relu(product + b))
    assert torch.equal(ops.resnet18_conv(g, biased, x, residual=res), (product + b) + res)
    full = ops.resnet18_conv(g, biased, x, residual=res, relu=True)
    assert torch.equal(full, torch.relu((product + b) + res)) and float(full.min()) == 0.0
    # and the folded weights themselves: against the float64 fold, as a product
    scale = (gamma.double() / torch.sqrt(var.double() + 1e-5)).cpu()
    want = F.conv2d(nchw(x).double(), w.cpu().double() * scale.view(-1, 1, 1, 1), None, stride, g.pad)
    cpu32 = F.conv2d(nchw(x), (w.cpu().double() * scale.view(-1, 1, 1, 1)).float(), None, stride, g.pad)
    bar(f'{name} folded', nchw(product), want, cpu32)


@pytest.mark.parametrize('shape', [(3, 14, 14, 64), (2, 7, 7, 8), (5, 5, 6, 4), (1, 1, 1, 4)])
def test_maxpool_is_exact(dev, shape):
    from arvae_amd import ops
    rs = np.random.RandomState(sum(shape))
    for shift in (0.0, -5.0):                                      # the second: every value negative, so padding-as-zero would win
        x = torch.from_numpy((rs.normal(0, 1, shape) + shift).astype(np.float32))
        if shift:
            assert float(x.max()) < 0.0
        got = ops.resnet18_maxpool(x.to(dev)).cpu()
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert tuple(got.shape) == tuple(want.shape) and torch.equal(got, want)


# ---- 3. the whole network -----------------------------------------------------------------------------------------------
def test_fixture_is_not_degenerate(fixture):
    assert len(set(fixture.pred64.tolist())) >= 8
    print(f'classes used {len(set(fixture.pred64.tolist()))}, smallest float64 top-2 margin {float(fixture.margin64.min()):.3e}, '
          f'torch-fp32 max logit error {fixture.logit_err32:.3e}')


@pytest.mark.parametrize('n', BATCHES)
def test_whole_network_against_float64(dev, fixture, model, n):
    x = torch.from_numpy(fixture.x[:n]).to(dev)
    logits, probs, pred = model.classify(x)
    bar(f'logits n={n}', logits.cpu(), fixture.logits64[:n], fixture.logits32[:n])
    p_hip = float((probs.cpu().double() - fixture.probs64[:n]).abs().max())
    p_cpu = float((fixture.probs32[:n].double() - fixture.probs64[:n]).abs().max())
    print(f'probs n={n}: max abs {p_hip:.3e} (torch fp32 {p_cpu:.3e})')
    assert p_hip <= 4.0 * p_cpu + 1e-7
    assert torch.equal(model(x), probs) and torch.equal(model.predict(x), pred)
    assert pred.dtype == torch.int64 and torch.equal(pred, probs.argmax(1))
    if n == max(BATCHES):
        assert len(set(fixture.pred64.tolist())) >= 8
        clear = resnet_ref.check_predictions(pred, fixture.logits64, fixture.logit_err32)
        print(f'{int(clear.sum())} of {n} rows over the margin')
        # the per-layer entry points run the same kernels on the same operands
        l2, p2, a2 = model.forward_layerwise(x)
        assert torch.equal(l2, logits) and torch.equal(p2, probs) and torch.equal(a2, pred)


# ---- 4. the preparation is not stale --------------------------------------------------------------------------------------
def test_preparation_follows_the_weights(dev, fixture):
    from arvae_amd.mnist_resnet import MnistResNet
    n = 16
    sd = {k: v.clone() for k, v in fixture.sd.items()}
    m = MnistResNet()
    m.load_state_dict(sd)
    m.to(dev).eval()
    x = torch.from_numpy(fixture.x[:n]).to(dev)
    first = m.classify(x)[0]
    again = m.classify(x)[0]
    assert torch.equal(first, again)                               # same input, same bits
    prep = m.prepared()
    assert m.prepared() is prep                                    # nothing changed: nothing rebuilt
    with torch.no_grad():
        m.layer2[0].bn1.running_var.mul_(1.75)                     # in place: _version moves, data_ptr does not
    changed = m.classify(x)[0]
    assert m.prepared() is not prep and not torch.equal(changed, first)
    sd['layer2.0.bn1.running_var'] = sd['layer2.0.bn1.running_var'] * 1.75
    xt = torch.from_numpy(fixture.x[:n])
    with torch.no_grad():
        want, cpu32 = resnet_ref.build(sd, torch.float64)(xt.double()), resnet_ref.build(sd, torch.float32)(xt)
    bar('logits after running_var *= 1.75', changed.cpu(), want, cpu32)
    m.load_state_dict(fixture.sd)                                  # copy_ into the same storage
    assert torch.equal(m.classify(x)[0], first)
    m.float().cpu().to(dev)                                        # moved: new storage
    assert torch.equal(m.classify(x)[0], first)


# ---- 5. get_resnet_accuracy end to end -------------------------------------------------------------------------------------
INTERP = {'area': (3, 0.5), 'length': (7, 0.4), 'thickness': (1, 0.3), 'slant': (12, 0.6), 'width': (5, 0.2), 'height': (9, 0.7),
          'mean': (-1, 0.45)}


def tiny_trainer(tmp_path, dev, n_test=40):
    from arvae_amd.data import MorphoMnistDataset
    from arvae_amd.image_vae import MnistVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    write_mnist(str(tmp_path), 48, n_test)
    ds = MorphoMnistDataset(root_dir=str(tmp_path / 'mnist_data' / 'plain'), device=dev)
    torch.manual_seed(0)
    trainer = ImageVAETrainer(ds, MnistVAE(), rand=0)
    trainer.cuda()
    return trainer, ds


def classifier_for(images, dev, seed=31):
    """a fixture classifier whose head is centred on `images` (n, 1, 28, 28)"""
    from arvae_amd.mnist_resnet import MnistResNet
    sd = resnet_ref.centre_head(resnet_ref.random_state_dict(seed), images)
    m = MnistResNet()
    m.load_state_dict(sd)
    return m.to(dev), sd


def test_get_resnet_accuracy_end_to_end(dev, tmp_path, monkeypatch):
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path / 'models'))
    trainer, ds = tiny_trainer(tmp_path, dev)
    images = torch.cat([b[0] for b in ds.data_loaders(16)[2]]).cpu().numpy()
    assert images.shape == (40, 1, 28, 28)
    resnet, sd = classifier_for(images, dev)
    trainer.metrics = {'interpretability': dict(INTERP)}
    decoded = []
    decode = trainer.model.decode

    def spy(z):
        decoded.append(z.detach().clone())
        return decode(z)
    monkeypatch.setattr(trainer.model, 'decode', spy)
    record = []
    result = trainer.get_resnet_accuracy(batch_size=16, resnet_model=resnet, record=record)
    assert set(result) == {'digit_pred_acc'} and set(result['digit_pred_acc']) == {'inputs', 'recons', 'interp'}
    # kinds and shapes: per batch 1 input, 1 reconstruction, 7 sweeps of 10 B; the last batch is ragged
    kinds = ['inputs', 'recons'] + [f'interp:{k}' for k in INTERP]
    sizes = (16, 16, 8)
    assert [r[0] for r in record] == kinds * 3
    labels_all = torch.cat([b[1] for b in ds.data_loaders(16)[2]])
    for i, (kind, imgs, labels, pred) in enumerate(record):
        b = sizes[i // 9]
        rows = b if kind in ('inputs', 'recons') else 10 * b
        want_labels = labels_all[sum(sizes[:i // 9]):sum(sizes[:i // 9]) + b]
        assert tuple(imgs.shape) == (rows, 1, 28, 28) and imgs.dtype == torch.float32 and imgs.is_cuda
        assert pred.dtype == torch.int64 and pred.is_cuda and tuple(pred.shape) == (rows,)
        assert torch.equal(labels, want_labels if rows == b else want_labels.repeat(10))
    assert torch.equal(record[0][1].cpu(), torch.from_numpy(images[:16]))
    # the sweeps: z.repeat(10, 1) with ONE column overwritten by linspace(-4, 4, 10).repeat_interleave(B); the seventh is column -1
    sweeps = [z for z in decoded if z.shape[0] in (160, 80)]
    assert len(sweeps) == 21
    for i, z in enumerate(sweeps):
        b = z.shape[0] // 10
        col = INTERP[list(INTERP)[i % 7]][0] % 16
        assert torch.equal(z[:, col], torch.linspace(-4.0, 4.0, 10, device=dev).repeat_interleave(b))
        others = [c for c in range(16) if c != col]
        assert torch.equal(z[:, others], z[:b, others].repeat(10, 1))
        if i % 7 == 6:
            assert col == 15 and not torch.equal(z[:, 15], sweeps[i - 1][:, 15])
    # the returned figures: the reference's arithmetic on the recorded predictions and labels
    acc = {'inputs': 0.0, 'recons': 0.0, 'interp': 0.0}
    for bi in range(3):
        rows = record[9 * bi:9 * bi + 9]
        per = [float((r[3] == r[2]).float().sum()) / r[3].shape[0] for r in rows]
        acc['inputs'] += per[0]
        acc['recons'] += per[1]
        acc['interp'] += sum(per[2:]) / 7
    for k in acc:
        assert abs(result['digit_pred_acc'][k] - acc[k] / 3) <= 1e-6, (k, result, acc)
    # the recorded predictions against the float64 restatement on the recorded images (rule 3 of the whole-network test)
    imgs = torch.cat([r[1] for r in record]).cpu()
    pred = torch.cat([r[3] for r in record]).cpu()
    with torch.no_grad():
        l64 = resnet_ref.build(sd, torch.float64)(imgs.double())
        l32 = resnet_ref.build(sd, torch.float32)(imgs)
    err32 = float((l32.double() - l64).abs().max())
    clear = resnet_ref.check_predictions(pred, l64, err32)
    print(f'{imgs.shape[0]} recorded images, {int(clear.sum())} over the margin, torch-fp32 max logit error {err32:.3e}, '
          f'classes predicted {sorted(set(pred.tolist()))}, figures {result["digit_pred_acc"]}')


# ---- 6. the CLI and results_dict.json --------------------------------------------------------------------------------------
TODAYS_KEYS = {'representations', 'interpretability', 'Corr_score', 'modularity_score', 'mig', 'SAP_score', 'test_loss', 'test_acc'}


def test_cli_and_results_dict(dev, tmp_path, monkeypatch):
    models = tmp_path / 'models'
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(models))
    trainer, ds = tiny_trainer(tmp_path, dev)
    trainer.model.save()                                           # the checkpoint `--test --rand 0` loads
    # without the classifier's checkpoint: the keys of today
    metrics = trainer.compute_eval_metrics(batch_size=16, random_state=0)
    results_fp = os.path.join(os.path.dirname(trainer.model.filepath), 'results_dict.json')
    assert set(metrics) == TODAYS_KEYS and set(json.load(open(results_fp))) == TODAYS_KEYS
    # with it: digit_pred_acc joins them, computed after test_model and written to the JSON
    images = torch.cat([b[0] for b in ds.data_loaders(16)[2]]).cpu().numpy()
    resnet, _ = classifier_for(images, dev)
    resnet.save()
    os.remove(results_fp)
    metrics = trainer.compute_eval_metrics(batch_size=16, random_state=0)
    written = json.load(open(results_fp))
    assert set(metrics) == TODAYS_KEYS | {'digit_pred_acc'} == set(written)
    assert set(written['digit_pred_acc']) == {'inputs', 'recons', 'interp'}
    assert all(0.0 <= v <= 1.0 for v in written['digit_pred_acc'].values())
    assert list(written)[-1] == 'digit_pred_acc'                   # where the reference puts it: after test_model's entries
    # the command line
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(models))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_image_vae.py'), '-d', 'mnist', '--test', '--rand', '0', '--batch_size', '16',
                        '--digit_acc'], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]
    assert set(summary['digit_pred_acc']) == {'inputs', 'recons', 'interp'} and 'interpretability' not in summary
    assert summary['digit_pred_acc']['inputs'] == pytest.approx(written['digit_pred_acc']['inputs'], abs=1e-6)

"""The figure path on the GPU: arvae_render_frames against the numpy restatement of tests/figure_cases.py (geometry: equality
on determined sources; quantisers: equality with the fp32-CPU bytes where the inputs sit away from the steps, the interval rule
q(v - TAU) <= byte <= q(v + TAU) elsewhere), its output bounds and stream, and the four figure methods of ImageVAETrainer and the
CLI's --gifs on tiny synthetic datasets."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import arvae_amd  # noqa: E402,F401
import figure_cases as fc  # noqa: E402
from test_data_gpu import write_dsprites, write_mnist  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def render(dev, src, cells, **kw):
    from arvae_amd import ops
    return ops.render_frames(torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).to(dev), cells, **kw).cpu().numpy()


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rgb', [True, False])
@pytest.mark.parametrize('shape', fc.SHAPES)
def test_geometry_is_exact(dev, shape, rgb):
    channels = 3 if rgb else 1
    seen = set()
    for i, (per_frame, nrow, padding, n_frames, pad_value, rounding) in enumerate(fc.geometry_cases()):
        v, b = fc.determined_images(shape, rounding, seed=i)
        cells = fc.geometry_cells(per_frame, n_frames, seed=100 + i)
        got = render(dev, v, cells, nrow=nrow, padding=padding, pad_value=pad_value, logits=False, rounding=rounding, rgb=rgb)
        pad = fc.effective_padding(n_frames, per_frame, padding)
        want = fc.grid(b, cells, nrow, pad, fc.pad_byte(pad_value, rounding), channels)
        assert got.dtype == np.uint8 and got.shape == want.shape, (per_frame, nrow, padding, n_frames)
        assert np.array_equal(got, want), (per_frame, nrow, padding, n_frames, pad_value, rounding)
        xmaps, ymaps, _, wg = fc.geometry(shape[0], shape[1], per_frame, nrow, pad)
        seen.add(('ragged', xmaps * ymaps > per_frame))
        seen.add(('blank', bool((cells < 0).any())))
        seen.add(('repeat', any(len(set(row[row >= 0])) < (row >= 0).sum() for row in cells)))
        seen.add(('odd row', (wg * channels) % 4 != 0))
        seen.add(('lone image', n_frames == 1 and per_frame == 1 and want.shape[1:3] == tuple(shape)))
    # what the table is there to reach
    assert {('ragged', True), ('blank', True), ('repeat', True), ('lone image', True)} <= seen
    if shape == (3, 5) or (shape == (28, 28) and rgb):
        assert ('odd row', True) in seen                 # rows of 57 / 19 bytes, and Morpho-MNIST's 546


def test_the_datasets_frame_sizes(dev):
    """Morpho-MNIST: six cells, 32 x 182, rows of 546 bytes (no multiple of 4); dSprites: five cells, 68 x 332"""
    for (h, w), per_frame, size in (((28, 28), 6, (32, 182)), ((64, 64), 5, (68, 332))):
        v, b = fc.determined_images((h, w), False, seed=3)
        cells = np.stack([np.arange(per_frame) % fc.N_IMAGES, (np.arange(per_frame) + 1) % fc.N_IMAGES])
        got = render(dev, v, cells, logits=False)         # the other defaults: nrow 8, padding 2, pad 1.0, truncating, RGB
        assert got.shape == (2,) + size + (3,)
        assert np.array_equal(got, fc.grid(b, cells, 8, 2, 255, 3))
    assert (182 * 3) % 4 != 0


# ---- 2. output bounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_output_stays_inside_its_buffer(dev, offset):
    """out inside a larger buffer, 64 guard bytes of 0xA5 either side; with offset 1..3 it starts off a 4-byte boundary.  Three RGB
    frames of 9 x 19 (rows of 57 bytes, 1539 bytes in all): head and tail of the output are partial words"""
    from arvae_amd import ops
    v, b = fc.determined_images((3, 5), False, seed=7)
    cells = fc.geometry_cells(5, 3, seed=8)
    want = fc.grid(b, cells, 3, 1, 255, 3)
    total = want.size
    assert total == 3 * 9 * 19 * 3 and total % 4 == 3
    buf = torch.full((64 + 4 + total + 64,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    out = buf[64 + offset:64 + offset + total]
    assert out.data_ptr() % 4 == offset
    got = ops.render_frames(torch.from_numpy(v).to(dev), cells, nrow=3, padding=1, logits=False, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    host = buf.cpu().numpy()
    assert np.all(host[:64 + offset] == 0xA5) and np.all(host[64 + offset + total:] == 0xA5)
    assert np.array_equal(host[64 + offset:64 + offset + total], want.ravel())


# ---- 3. quantisers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(fc.quantiser_cases()))
def test_quantiser_cases_equal_the_fp32_cpu_bytes(dev, name):
    src, logits, rounding, expect = fc.quantiser_cases()[name]
    cells = np.arange(src.shape[0])[None]
    for rgb in (True, False):
        got = render(dev, src, cells, logits=logits, rounding=rounding, rgb=rgb)       # (one cell, one frame: no padding)
        assert got.shape == (1,) + src.shape[1:] + (3 if rgb else 1,)
        for c in range(got.shape[3]):
            assert np.array_equal(got[0, :, :, c], expect[0]), (name, rgb, got[0, :, :, c].ravel(), expect.ravel())
    assert np.array_equal(fc.fp32_cpu_bytes(src, logits, rounding), expect)


@pytest.mark.parametrize('rounding', [False, True])
def test_random_logits_under_the_interval_rule(dev, rounding):
    src = fc.random_logits()
    cells = np.arange(64)[None]
    got = render(dev, src, cells, nrow=8, padding=2, pad_value=1.0, logits=True, rounding=rounding, rgb=True)
    lo, hi = fc.interval(src, True, rounding)
    lo, hi = fc.grid(lo, cells, 8, 2, 255, 3), fc.grid(hi, cells, 8, 2, 255, 3)
    cpu = fc.grid(fc.fp32_cpu_bytes(src, True, rounding), cells, 8, 2, 255, 3)
    assert got.shape == lo.shape == (1, 8 * 30 + 2, 8 * 30 + 2, 3)
    outside = (got < lo) | (got > hi)
    print(f'rounding {rounding}: {int(outside.sum())} bytes outside the interval, {int((got != cpu).sum())} of {got.size} differ from '
          f'the fp32-CPU bytes, {int((lo != hi).sum())} undetermined')
    assert not outside.any()


# ---- 4. stream --------------------------------------------------------------------------------------------------------------------
def test_side_stream_gives_the_same_bytes(dev):
    from arvae_amd import ops
    src = torch.from_numpy(fc.random_logits()).to(dev)
    cells = np.arange(64).reshape(8, 8)
    want = ops.render_frames(src, cells).cpu()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ops.render_frames(src, cells)
    s.synchronize()
    assert torch.equal(got.cpu(), want)


# ---- 5. the trainer's figure methods ----------------------------------------------------------------------------------------------
INTERP = {'mnist': {'area': (3, 0.5), 'length': (7, 0.4), 'thickness': (1, 0.3), 'slant': (12, 0.6), 'width': (5, 0.2),
                    'height': (9, 0.7), 'mean': (-1, 0.45)},
          'dsprites': {'shape': (2, 0.5), 'scale': (0, 0.4), 'orientation': (7, 0.3), 'posx': (4, 0.6), 'posy': (9, 0.2),
                       'mean': (-1, 0.4)}}
FRAME = {'mnist': (32, 182), 'dsprites': (68, 332)}


def tiny_trainer(kind, tmp_path, dev):
    """Xavier-initialised model on a synthetic dataset; -> (trainer, the evaluation split's images as bytes (n, hw, hw))"""
    from arvae_amd.data import DspritesDataset, MorphoMnistDataset
    from arvae_amd.image_vae import DspritesVAE, MnistVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    torch.manual_seed(0)
    if kind == 'mnist':
        imgs = write_mnist(str(tmp_path), 48, 40)['t10k'][0]
        ds = MorphoMnistDataset(root_dir=str(tmp_path / 'mnist_data' / 'plain'), device=dev)
        trainer = ImageVAETrainer(ds, MnistVAE(), rand=0)
    else:
        imgs, _ = write_dsprites(str(tmp_path), 200)
        imgs = imgs[int((0.80 + 0.15) * 200):] * np.uint8(255)
        ds = DspritesDataset(path=str(tmp_path / 'dsprites_ndarray_co1sh3sc6or40x32y32_64x64.npz'), device=dev)
        trainer = ImageVAETrainer(ds, DspritesVAE(), rand=0)
    trainer.cuda()
    return trainer, imgs


class DecodeSpy:
    """records what the model's decoder was given and what it returned"""

    def __init__(self, model, monkeypatch):
        self.calls = []
        decode = model.decode

        def spy(z):
            out = decode(z)
            self.calls.append((z.detach().cpu().numpy().copy(), out.detach().cpu().numpy()[:, 0].copy()))
            return out
        monkeypatch.setattr(model, 'decode', spy)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == 'RGB', path
        return np.asarray(im).copy()


def assert_within(pixels, logits, cells, nrow, padding, rounding, what):
    """pixels (F, Hg, Wg, 3) against the frames the restatement builds from the decoder's logits"""
    lo, hi = fc.interval(logits, True, rounding)
    pad = fc.pad_byte(1.0, rounding)
    lo, hi = fc.grid(lo, cells, nrow, padding, pad, 3), fc.grid(hi, cells, nrow, padding, pad, 3)
    assert pixels.shape == lo.shape, (what, pixels.shape, lo.shape)
    outside = (pixels < lo) | (pixels > hi)
    print(f'{what}: {pixels.shape}, {int(outside.sum())} bytes outside the interval, {int((lo != hi).sum())} undetermined, '
          f'bytes {pixels.min()}..{pixels.max()}')
    assert not outside.any(), what


@pytest.mark.parametrize('kind', ['dsprites', 'mnist'])
def test_trainer_figures(dev, tmp_path, monkeypatch, kind):
    from PIL import Image
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path / 'models'))
    trainer, images = tiny_trainer(kind, tmp_path, dev)
    model = trainer.model
    interp = INTERP[kind]
    trainer.metrics = {'interpretability': dict(interp)}
    attrs = [a for a in trainer.attr_dict if a not in ('digit_identity', 'color')]
    zdim = model.z_dim
    results = os.path.join(os.path.dirname(model.filepath), 'results')
    hw = images.shape[1]
    model.eval()
    with torch.no_grad():                                # the posterior means of evaluation samples 1 and 2
        x = torch.from_numpy(images[:3].astype(np.float32) / np.float32(255.0) if kind == 'dsprites' else
                             images[:3].astype(np.float32) * np.float32(1.0 / 255.0)).to(dev).view(3, 1, hw, hw)
        mu = model.encode(x).loc.cpu().numpy()
    model._masks = None
    spy = DecodeSpy(model, monkeypatch)
    sweep = np.linspace(-4.0, 4.0, 3, dtype=np.float32)

    # create_latent_gifs: one decoder batch, attribute-major; 3 frames with cell a = attribute a at sweep point n
    paths = trainer.create_latent_gifs(sample_id=1, num_points=3, deterministic=True)
    assert paths == [os.path.join(results, f'gif_interpolations_{kind}_1.gif')] and os.path.exists(paths[0])
    calls = spy.take()
    assert [c[0].shape for c in calls] == [(1, zdim), (3 * len(attrs), zdim)]           # the reconstruction, then every sweep at once
    z, logits = calls[1]
    for a, attr in enumerate(attrs):
        d = interp[attr][0]
        rows = z[3 * a:3 * a + 3]
        assert np.array_equal(rows[:, d], sweep), attr
        others = [c for c in range(zdim) if c != d]
        assert np.allclose(rows[:, others], np.repeat(mu[1:2, others], 3, axis=0), rtol=0, atol=1e-4), attr      # the mean, not a sample
    with Image.open(paths[0]) as im:
        assert im.n_frames == 3 and im.size == FRAME[kind][::-1] and im.info['duration'] == 100 and im.info['loop'] == 0
        frames = []
        for i in range(3):
            im.seek(i)
            frames.append(np.asarray(im.convert('RGB')).copy())
    cells = np.arange(3 * len(attrs)).reshape(len(attrs), 3).T
    assert_within(np.stack(frames), logits, cells, 8, 2, False, f'{kind} gif')

    # plot_latent_interpolations: one row per sample; sample 500 is past the end of the split and is left out
    attr = attrs[2]
    paths = trainer.plot_latent_interpolations(attr, num_points=3, sample_ids=(2, 500), deterministic=True)
    assert paths == [os.path.join(results, n) for n in (f'latent_interpolations_{attr}_2.png', 'original_2.png', 'recons_2.png')]
    calls = spy.take()
    assert [c[0].shape for c in calls] == [(1, zdim), (3, zdim)]
    assert np.allclose(calls[0][0], mu[2:3], rtol=0, atol=1e-4) and np.array_equal(calls[1][0][:, interp[attr][0]], sweep)
    assert_within(read_png(paths[0])[None], calls[1][1], np.arange(3)[None], 3, 2, True, f'{kind} interpolation row')
    original = read_png(paths[1])
    assert original.shape == (hw, hw, 3) and all(np.array_equal(original[:, :, c], images[2]) for c in range(3))    # unpadded, the input's bytes
    assert_within(read_png(paths[2])[None], calls[0][1], np.zeros((1, 1), int), 1, 0, True, f'{kind} reconstruction')

    # the same row truncated, as the GIF frames are
    paths = trainer.plot_latent_interpolations(attr, num_points=3, sample_ids=(2,), deterministic=True, rounding=False)
    calls = spy.take()
    assert_within(read_png(paths[0])[None], calls[1][1], np.arange(3)[None], 3, 2, False, f'{kind} interpolation row, truncated')

    # plot_latent_interpolations2d: 'ij': the first attribute's dimension changes from row to row, the second's along a row
    a1, a2 = ('slant', 'thickness') if kind == 'mnist' else ('posx', 'posy')
    paths = trainer.plot_latent_interpolations2d(a1, a2, num_points=3, sample_id=1, deterministic=True)
    assert paths == [os.path.join(results, n) for n in (f'latent_interpolations_2d_({a1},{a2})_1.png', 'original_1.png', 'recons_1.png')]
    calls = spy.take()
    z, logits = calls[1]
    assert z.shape == (9, zdim)
    assert np.array_equal(z[:, interp[a1][0]], np.repeat(sweep, 3)) and np.array_equal(z[:, interp[a2][0]], np.tile(sweep, 3))
    grid2d = read_png(paths[0])
    assert grid2d.shape == (3 * (hw + 2) + 2, 3 * (hw + 2) + 2, 3)
    assert_within(grid2d[None], logits, np.arange(9)[None], 3, 2, True, f'{kind} 2-d grid')
    assert all(np.array_equal(read_png(paths[1])[:, :, c], images[1]) for c in range(3))

    # plot_latent_reconstructions: the first evaluation batch and its reconstructions, one row each
    paths = trainer.plot_latent_reconstructions(num_points=4, deterministic=True)
    assert paths == [os.path.join(results, 'r_original_0.png'), os.path.join(results, 'r_recons_0.png')]
    calls = spy.take()
    assert len(calls) == 1 and calls[0][0].shape == (4, zdim)
    assert np.array_equal(read_png(paths[0]), fc.grid(images[:4], np.arange(4)[None], 4, 2, 255, 3)[0])
    assert_within(read_png(paths[1])[None], calls[0][1], np.arange(4)[None], 4, 2, True, f'{kind} reconstructions')

    # the default takes the sampled code of a forward pass, as the reference does: two calls differ
    first = trainer.create_latent_gifs(sample_id=0, num_points=2)
    z_a = spy.take()[1][0]
    trainer.create_latent_gifs(sample_id=0, num_points=2)
    z_b = spy.take()[1][0]
    assert os.path.exists(first[0]) and not np.array_equal(z_a, z_b)


def test_figures_need_the_interpretability_metric(dev, tmp_path, monkeypatch):
    """the dimensions come from results_dict.json when the trainer has not computed the metrics itself"""
    import json
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path / 'models'))
    trainer, _ = tiny_trainer('dsprites', tmp_path, dev)
    folder = os.path.dirname(trainer.model.filepath)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, 'results_dict.json'), 'w') as f:
        json.dump({'interpretability': {k: list(v) for k, v in INTERP['dsprites'].items()}}, f)
    spy = DecodeSpy(trainer.model, monkeypatch)
    paths = trainer.create_latent_gifs(sample_id=3, num_points=2, deterministic=True)
    assert os.path.exists(paths[0]) and trainer.metrics['interpretability']['posx'] == [4, 0.6]
    z = spy.take()[1][0]
    assert z.shape == (10, 10) and np.array_equal(z[6:8, 4], [-4.0, 4.0])               # posx is the fourth attribute: rows 6, 7
    assert trainer.create_latent_gifs(sample_id=10, num_points=2) == []                   # the split has ten items


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_gifs(dev, tmp_path, monkeypatch):
    from PIL import Image
    models = tmp_path / 'models'
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(models))
    trainer, _ = tiny_trainer('mnist', tmp_path, dev)
    trainer.model.save()                                 # the checkpoint `--test --rand 0` loads
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(models))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_image_vae.py'), '-d', 'mnist', '--test', '--rand', '0', '--batch_size', '16',
                        '--gifs'], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    results = os.path.join(os.path.dirname(trainer.model.filepath), 'results')
    assert sorted(os.listdir(results)) == [f'gif_interpolations_mnist_{i}.gif' for i in (0, 1, 4)]
    for name in os.listdir(results):
        assert f'wrote {os.path.join(results, name)}' in r.stdout
        with Image.open(os.path.join(results, name)) as im:
            assert im.n_frames == 10 and im.size == (182, 32)

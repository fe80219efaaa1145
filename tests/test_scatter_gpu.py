"""Scatter figures on the GPU: arvae_render_scatter byte for byte against the numpy restatement of tests/scatter_cases.py (every case
of its table, the order of the input, the output's bounds at every start offset, the stream), MeasureVAETrainer.compute_latent_surface
against the public calls it composes, plot_latent_surface and both trainers' plot_data_dist read back from the files they write, and
the command lines' --data_dist and --surfaces."""
import json
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
import scatter_cases as sc  # noqa: E402
from test_data_gpu import write_folk  # noqa: E402
from test_pianoroll_gpu import read_png, tiny_trainer  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = sc.raster_cases()
ATTRS = ('rhy_complexity', 'pitch_range', 'note_density', 'contour')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def render(dev, points, values, xlim, ylim, vmin=None, vmax=None, **look):
    from arvae_amd import ops
    return ops.render_scatter(torch.from_numpy(np.ascontiguousarray(points)).to(dev), torch.from_numpy(np.ascontiguousarray(values)).to(dev),
                              xlim, ylim, vmin, vmax, **look)


def differences(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:5].tolist()


# ---- 1. the raster ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_raster_is_exact(dev, name):
    """every byte of every figure of the case: no pixel is left out of the comparison"""
    points, values, xlim, ylim, vmin, vmax, look = sc.case_inputs(CASES[name])
    want = sc.scatter(points, values, xlim, ylim, vmin, vmax, **look)
    got = render(dev, points, values, xlim, ylim, vmin, vmax, **look).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), differences(got, want)


def test_default_look(dev):
    """every keyword at its default: 485 x 360, radius 2, alpha 0.5, the bounds found from the values, 'dimension: 0' / 'dimension: 1'"""
    rng = np.random.RandomState(3)
    points, values = (rng.randn(2, 500, 2) * 1.5).astype(np.float32), rng.randn(2, 500).astype(np.float32)
    values[0, 7], values[1, :] = np.nan, 0.75            # a missing value; a figure whose values are all the same
    got = render(dev, points, values, (-4.0, 4.0), (-4.0, 4.0)).cpu().numpy()
    assert got.shape == (2, 360, 485, 3)
    want = sc.scatter(points, values, (-4.0, 4.0), (-4.0, 4.0))
    assert np.array_equal(got, want), differences(got, want)
    # no points at all: the empty figure
    empty = render(dev, np.zeros((1, 0, 2), np.float32), np.zeros((1, 0), np.float32), (-4.0, 4.0), (-4.0, 4.0)).cpu().numpy()
    assert np.array_equal(empty, sc.scatter(np.zeros((1, 0, 2), np.float32), np.zeros((1, 0), np.float32), (-4.0, 4.0), (-4.0, 4.0)))


@pytest.mark.parametrize('name', ['dense_r5_a0.5', 'dense_r2_a0.3', 'one_pixel_300', 'n1000_f1'])
def test_order_of_the_input_decides(dev, name):
    """the reversed input gives the restatement of the reversed input, and another picture than the forward one"""
    points, values, xlim, ylim, vmin, vmax, look = sc.case_inputs(CASES[name])
    points, values = points[:, ::-1], values[:, ::-1]
    vmin, vmax = (0.0, 1.0) if vmin is None else (vmin, vmax)
    forward = sc.scatter(points[:, ::-1], values[:, ::-1], xlim, ylim, vmin, vmax, **look)
    want = sc.scatter(points, values, xlim, ylim, vmin, vmax, **look)
    got = render(dev, points, values, xlim, ylim, vmin, vmax, **look).cpu().numpy()
    assert np.array_equal(got, want), differences(got, want)
    assert not np.array_equal(got, forward)


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_output_stays_inside_its_buffer(dev, offset):
    """out inside a larger buffer, 64 guard bytes of 0xA5 either side; with offset 1..3 it starts off a 4-byte boundary.  Three figures
    of 226 x 106 (rows of 678 bytes: every row starts at another alignment; a whole number of words in all) and one of 227 x 107 (72867
    bytes: the last word is partial at every offset)"""
    from arvae_amd import ops
    rng = np.random.RandomState(8)
    for f, width, height in ((3, 226, 106), (1, 227, 107)):
        points, values = (rng.randn(f, 200, 2) * 2).astype(np.float32), rng.rand(f, 200).astype(np.float32)
        look = dict(width=width, height=height, radius=5, alpha=0.5)
        want = sc.scatter(points, values, (-4.0, 4.0), (-4.0, 4.0), 0.0, 1.0, **look)
        total = want.size
        assert (3 * width) % 4 != 0 and (total % 4 != 0) == (f == 1)
        buf = torch.full((64 + 4 + total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 4 == 0
        out = buf[64 + offset:64 + offset + total]
        pts, val = torch.from_numpy(points).to(dev), torch.from_numpy(values).to(dev)
        got = ops.render_scatter(pts, val, (-4.0, 4.0), (-4.0, 4.0), 0.0, 1.0, out=out, **look)
        assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 4 == offset
        assert np.array_equal(got.cpu().numpy(), want), differences(got.cpu().numpy(), want)
        host = buf.cpu().numpy()
        assert np.all(host[:64 + offset] == 0xA5) and np.all(host[64 + offset + total:] == 0xA5)
        strided = torch.zeros(2 * total, dtype=torch.uint8, device=dev)[::2]             # the right size, not dense: refused before the launch
        with pytest.raises(ValueError, match='contiguous'):
            ops.render_scatter(pts, val, (-4.0, 4.0), (-4.0, 4.0), 0.0, 1.0, out=strided, **look)


def test_launch_goes_to_the_current_stream(dev):
    """The launch is captured into a HIP graph on a stream of its own (arvae_amd.graphed.Capture): a capture records only what is
    launched on the capturing stream and runs nothing, so an output that holds the right bytes after a replay -- and only after it
    -- came from a launch on the current stream.  Then the same on a plain side stream."""
    from arvae_amd import ops
    from arvae_amd.graphed import Capture
    rng = np.random.RandomState(4)
    points, values = (rng.randn(4, 700, 2) * 1.5).astype(np.float32), rng.rand(4, 700).astype(np.float32)
    want = sc.scatter(points, values, (-4.0, 4.0), (-4.0, 4.0), 0.0, 1.0, **sc.SMALL)
    pts, val = torch.from_numpy(points).to(dev), torch.from_numpy(values).to(dev)
    frames = torch.full(want.shape, 0xA5, dtype=torch.uint8, device=dev)
    cap = Capture(device=dev)
    cap.capture(lambda: ops.render_scatter(pts, val, (-4.0, 4.0), (-4.0, 4.0), 0.0, 1.0, out=frames, **sc.SMALL))      # (bounds given: no host read)
    torch.cuda.synchronize()
    assert bool((frames == 0xA5).all())                  # captured, not run
    cap.replay()
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ops.render_scatter(pts, val, (-4.0, 4.0), (-4.0, 4.0), 0.0, 1.0, **sc.SMALL)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


# ---- 2. the trainers ----------------------------------------------------------------------------------------------------------------------
def reference_grid(grid_res):
    x = torch.arange(-5., 5., grid_res)
    z1, z2 = torch.meshgrid([x, x], indexing='ij')       # (the reference's call predates the keyword; 'ij' is what it got)
    return z1, z2


@pytest.mark.parametrize('grid_res,n', [(2.5, 4), (0.5, 20)])
def test_compute_latent_surface(dev, tmp_path, monkeypatch, grid_res, n):
    trainer = tiny_trainer(tmp_path, monkeypatch)
    base = torch.from_numpy(np.random.RandomState(2).randn(16).astype(np.float32))
    dim1, dim2 = 12, 3
    grid, labels = trainer.compute_latent_surface(dim1, dim2, grid_res, base, chunk=7)
    assert grid.shape == (n, n, 2) and labels.shape == (n, n, 4) and grid.is_cuda and labels.is_cuda and labels.dtype == torch.float32
    z1, z2 = reference_grid(grid_res)
    assert z1.shape == (n, n) and torch.equal(grid[:, :, 0].cpu(), z1) and torch.equal(grid[:, :, 1].cpu(), z2)
    # the composition of the public calls, over the same chunks
    z = base.reshape(1, -1).repeat(n * n, 1)
    z[:, dim1], z[:, dim2] = z1.reshape(-1), z2.reshape(-1)
    z = z.to(dev)
    assert (n * n) % 7 != 0
    want = torch.cat([trainer.compute_attribute_labels(trainer.decode_latent_codes(z[at:at + 7])[1].reshape(-1, 24)) for at in range(0, n * n, 7)])
    assert torch.equal(labels.reshape(n * n, 4), want)
    assert len(torch.unique(labels.reshape(-1, 4), dim=0)) > 1                     # (the surface is not flat)
    # one chunk for all codes gives the same labels; a selection of attributes is those columns
    whole, picked = trainer.compute_latent_surface(dim1, dim2, grid_res, base)[1], trainer.compute_latent_surface(
        dim1, dim2, grid_res, base, ['contour', 'pitch_range'], chunk=7)[1]
    assert torch.equal(whole, labels) and torch.equal(picked, labels[:, :, [3, 1]])
    # without a base code: one draw from the library's generator, which a seed reproduces
    from arvae_amd import ops
    ops.rng_reseed(5)
    first = trainer.compute_latent_surface(0, 1, grid_res)[1]
    ops.rng_reseed(5)
    assert torch.equal(trainer.compute_latent_surface(0, 1, grid_res)[1], first)
    with pytest.raises(ValueError):
        trainer.compute_latent_surface(0, 1, grid_res, base[:5])


def test_plot_latent_surface(dev, tmp_path, monkeypatch):
    from arvae_amd import ops
    trainer = tiny_trainer(tmp_path, monkeypatch)
    folder = os.path.join(os.path.dirname(trainer.model.filepath), 'results')
    base = np.random.RandomState(2).randn(16).astype(np.float32)
    launches, render_scatter = [], ops.render_scatter
    monkeypatch.setattr(ops, 'render_scatter', lambda *a, **kw: launches.append(render_scatter(*a, **kw)) or launches[-1])
    grid, labels = trainer.compute_latent_surface(12, 3, 0.5, base)
    points = grid.reshape(1, 400, 2).cpu().numpy()
    path = trainer.plot_latent_surface('contour', 12, 3, grid_res=0.5, base_code=base)
    assert path == os.path.join(folder, 'latent_surface_contour.png') and len(launches) == 1
    want = sc.scatter(points, labels[:, :, 3].reshape(1, 400).cpu().numpy(), (-5.0, 5.0), (-5.0, 5.0), labels=('dimension: 12', 'dimension: 3'))
    png = read_png(path)
    assert png.shape == (360, 485, 3) and np.array_equal(png, want[0]), differences(png, want[0])
    # a list: one decode pass over the plane and one launch for all figures; a look of the caller's
    decodes, decode = [], trainer.decode_latent_codes
    monkeypatch.setattr(trainer, 'decode_latent_codes', lambda z, *a, **kw: decodes.append(z.shape[0]) or decode(z, *a, **kw))
    paths = trainer.plot_latent_surface(list(ATTRS), 12, 3, grid_res=0.5, base_code=base, radius=5, alpha=1.0, **sc.SMALL)
    assert paths == [os.path.join(folder, f'latent_surface_{a}.png') for a in ATTRS] and len(launches) == 2 and decodes == [400]
    assert sorted(os.listdir(folder)) == sorted(os.path.basename(p) for p in paths)
    want = sc.scatter(np.repeat(points, 4, 0), labels.reshape(400, 4).t().cpu().numpy(), (-5.0, 5.0), (-5.0, 5.0), radius=5, alpha=1.0,
                      labels=('dimension: 12', 'dimension: 3'), **sc.SMALL)
    for i, p in enumerate(paths):
        png = read_png(p)
        assert png.shape == (106, 226, 3) and np.array_equal(png, want[i]), (ATTRS[i], differences(png, want[i]))
    # a dimension a name: every distinct plane is decoded once, around the same base code
    decodes.clear()
    paths = trainer.plot_latent_surface(['contour', 'note_density', 'pitch_range'], [12, 5, 12], 3, grid_res=2.5, base_code=base, **sc.SMALL)
    assert decodes == [16, 16] and len(launches) == 3
    other = trainer.compute_latent_surface(5, 3, 2.5, base, ['note_density'])[1]
    coarse = trainer.compute_latent_surface(12, 3, 2.5, base)
    values = np.stack([coarse[1][:, :, 3].reshape(-1).cpu().numpy(), other.reshape(-1).cpu().numpy(), coarse[1][:, :, 1].reshape(-1).cpu().numpy()])
    want = sc.scatter(np.repeat(coarse[0].reshape(1, 16, 2).cpu().numpy(), 3, 0), values, (-5.0, 5.0), (-5.0, 5.0),
                      labels=[('dimension: 12', 'dimension: 3'), ('dimension: 5', 'dimension: 3'), ('dimension: 12', 'dimension: 3')], **sc.SMALL)
    assert all(np.array_equal(read_png(p), want[i]) for i, p in enumerate(paths))
    with pytest.raises(ValueError):
        trainer.plot_latent_surface('loudness')


def test_measure_plot_data_dist(dev, tmp_path, monkeypatch):
    trainer = tiny_trainer(tmp_path, monkeypatch)
    folder = os.path.join(os.path.dirname(trainer.model.filepath), 'results')
    rng = np.random.RandomState(6)
    codes, attrs = (rng.randn(300, 16) * 1.7).astype(np.float32), rng.rand(300, 4).astype(np.float32)
    path = trainer.plot_data_dist(codes, attrs, 'note_density', 5, 15)
    assert path == os.path.join(folder, 'data_dist_note_density.png')
    want = sc.scatter(codes[None][:, :, [5, 15]], attrs[None, :, 2], (-4.0, 4.0), (-4.0, 4.0), labels=('dimension: 5', 'dimension: 15'))
    png = read_png(path)
    assert png.shape == (360, 485, 3) and np.array_equal(png, want[0]), differences(png, want[0])
    assert np.array_equal(read_png(trainer.plot_data_dist(codes, attrs, 'contour')), sc.scatter(codes[None][:, :, [0, 1]], attrs[None, :, 3],
                                                                                             (-4.0, 4.0), (-4.0, 4.0))[0])
    from arvae_amd import ops
    launches, render_scatter = [], ops.render_scatter
    monkeypatch.setattr(ops, 'render_scatter', lambda *a, **kw: launches.append(render_scatter(*a, **kw)) or launches[-1])
    dims = [3, 7, 1, 12]
    paths = trainer.plot_data_dist(codes, attrs, list(ATTRS), dims, 15, **sc.SMALL)
    assert paths == [os.path.join(folder, f'data_dist_{a}.png') for a in ATTRS] and len(launches) == 1 and launches[0].shape == (4, 106, 226, 3)
    want = sc.scatter(np.stack([codes[:, [d, 15]] for d in dims]), attrs.T, (-4.0, 4.0), (-4.0, 4.0),
                      labels=[(f'dimension: {d}', 'dimension: 15') for d in dims], **sc.SMALL)
    assert all(np.array_equal(read_png(p), want[i]) for i, p in enumerate(paths))
    with pytest.raises(ValueError):
        trainer.plot_data_dist(codes, attrs, 'loudness')


def test_image_plot_data_dist(dev, tmp_path, monkeypatch):
    from test_figures_gpu import tiny_trainer as tiny_image_trainer
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path / 'models'))
    trainer, _ = tiny_image_trainer('dsprites', tmp_path, dev)
    folder = os.path.join(os.path.dirname(trainer.model.filepath), 'results')
    rng = np.random.RandomState(7)
    codes = (rng.randn(200, 10) * 1.7).astype(np.float32)
    relevant, labels = rng.rand(200, 5).astype(np.float32), rng.rand(200, 6).astype(np.float32)      # compute_representations' columns; the labels
    path = trainer.plot_data_dist(codes, relevant, 'posx', 4, 9)
    assert path == os.path.join(folder, 'data_dist_posx.png')
    want = sc.scatter(codes[None][:, :, [4, 9]], relevant[None, :, 3], (-4.0, 4.0), (-4.0, 4.0), labels=('dimension: 4', 'dimension: 9'))
    assert np.array_equal(read_png(path), want[0])
    names = ['shape', 'scale', 'orientation', 'posx', 'posy']
    paths = trainer.plot_data_dist(codes, labels, names, [2, 0, 7, 4, 9], 8, **sc.SMALL)
    assert paths == [os.path.join(folder, f'data_dist_{a}.png') for a in names]
    want = sc.scatter(np.stack([codes[:, [d, 8]] for d in (2, 0, 7, 4, 9)]), labels[:, 1:].T, (-4.0, 4.0), (-4.0, 4.0),
                      labels=[(f'dimension: {d}', 'dimension: 8') for d in (2, 0, 7, 4, 9)], **sc.SMALL)
    assert all(np.array_equal(read_png(p), want[i]) for i, p in enumerate(paths))
    with pytest.raises(ValueError):
        trainer.plot_data_dist(codes, relevant, 'color')
    with pytest.raises(ValueError):
        trainer.plot_data_dist(codes, labels[:, :3], 'posx')


# ---- 3. the command lines -------------------------------------------------------------------------------------------------------------------
def check_figure(path):
    """a file of the default canvas with the frame and the colour bar where the geometry puts them, and markers inside"""
    png = read_png(path)
    assert png.shape == (360, 485, 3)
    g = sc.geometry()
    assert (png[g['py0'] - 1, g['px0'] - 1:g['px0'] + g['pw'] + 1] == 0).all() and (png[g['py0']:g['py0'] + g['ph'], g['px0'] - 1] == 0).all()
    bar = png[g['py0']:g['py0'] + g['ph'], g['bar_x']:g['bar_x'] + g['bar_w']]
    assert (bar[0] == sc.VIRIDIS[255]).all() and (bar[-1] == sc.VIRIDIS[0]).all()
    assert (png[g['py0']:g['py0'] + g['ph'], g['px0']:g['px0'] + g['pw']] != 255).any()
    return png


def test_measure_cli_writes_data_dist_and_surfaces(dev, tmp_path):
    """on write_folk data: a one-epoch run with --data_dist --surfaces writes the files its summary lists, in a child process"""
    write_folk(str(tmp_path), 400)
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(tmp_path / 'models'))
    args = ['--num_epochs', '1', '--data_dist', '--surfaces', '--batch_size', '16', '--rand', '1', '-r', 'all', '--encoder_hidden_size', '64',
            '--decoder_hidden_size', '64']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + args, capture_output=True, text=True, timeout=600,
                       env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]
    folder = os.path.dirname(summary['data_dist'][0])
    assert folder.endswith('results')
    assert summary['data_dist'] == [os.path.join(folder, f'data_dist_{a}.png') for a in ATTRS]
    assert summary['surfaces'] == [os.path.join(folder, f'latent_surface_{a}.png') for a in ATTRS]
    assert sorted(os.listdir(folder)) == sorted(os.path.basename(p) for p in summary['data_dist'] + summary['surfaces'])
    assert 'interpretability' not in summary             # (the metrics were computed for the planes, not asked for)
    for path in summary['data_dist']:
        check_figure(path)
    g = sc.geometry()
    for path in summary['surfaces']:                     # 200 x 200 opaque-enough discs over -5..5: no white left well inside the plot area
        png = check_figure(path)
        assert (png[g['py0'] + 20:g['py0'] + g['ph'] - 20, g['px0'] + 20:g['px0'] + g['pw'] - 20] != 255).any(2).all()


def test_image_cli_writes_data_dist(dev, tmp_path, monkeypatch):
    from test_figures_gpu import tiny_trainer as tiny_image_trainer
    models = tmp_path / 'models'
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(models))
    trainer, _ = tiny_image_trainer('mnist', tmp_path, dev)
    trainer.model.save()                                 # the checkpoint `--test --rand 0` loads
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(models))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_image_vae.py'), '-d', 'mnist', '--test', '--rand', '0', '--batch_size', '16',
                        '--data_dist'], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    results = os.path.join(os.path.dirname(trainer.model.filepath), 'results')
    names = ['area', 'length', 'thickness', 'slant', 'width', 'height']
    assert sorted(os.listdir(results)) == sorted(f'data_dist_{a}.png' for a in names)
    for a in names:
        assert f'wrote {os.path.join(results, f"data_dist_{a}.png")}' in r.stdout
        check_figure(os.path.join(results, f'data_dist_{a}.png'))

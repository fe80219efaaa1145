"""The figure path without a GPU: the ABI of the render entry points and their host checks, the Python wrapper's refusals, the
numpy restatement of the grid against logging_utils.image_grid, the GIF writer's round trip, the CLI switches, and the
acceptance rule's own honesty (tests/figure_cases.py): the fp32-CPU bytes pass it and it decides all but 0.1 % of a case's
pixels."""
import ctypes
import os
import re
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


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_render_entry_points_are_declared_exported_and_bound(lib):
    from arvae_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'arvae_hip.h')).read()
    assert re.search(r'#define ARVAE_ABI_VERSION 16\b', header) and _lib.ABI_VERSION == 16 and lib.arvae_abi_version() == 16
    for name in ('arvae_render_frame_bytes', 'arvae_render_frames'):
        assert re.search(r'\b' + name + r'\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    from arvae_amd import ops
    for flag in ('SRC_LOGITS', 'ROUND', 'RGB'):
        value = int(re.search(rf'#define ARVAE_RENDER_{flag} (\d+)', header).group(1))
        assert getattr(ops, 'RENDER_' + flag) == value


def test_frame_bytes_equals_the_restatement(lib):
    for (h, w) in fc.SHAPES:
        for per_frame, nrow, padding, _, _, _ in fc.geometry_cases():
            _, _, hg, wg = fc.geometry(h, w, per_frame, nrow, padding)
            for channels in (1, 3):
                assert lib.arvae_render_frame_bytes(h, w, per_frame, nrow, padding, channels) == hg * wg * channels
    # the figures of the two datasets: six Morpho-MNIST cells, five dSprites cells
    assert lib.arvae_render_frame_bytes(28, 28, 6, 8, 2, 3) == 32 * 182 * 3
    assert lib.arvae_render_frame_bytes(64, 64, 5, 8, 2, 3) == 68 * 332 * 3
    assert lib.arvae_render_frame_bytes(28, 28, 6, 8, 2, 2) == -1 and b'channels' in lib.arvae_last_error_string()
    assert lib.arvae_render_frame_bytes(0, 28, 6, 8, 2, 3) == -1 and lib.arvae_render_frame_bytes(28, 28, 6, 0, 2, 3) == -1
    assert lib.arvae_render_frame_bytes(28, 28, 6, 8, -1, 3) == -1
    assert lib.arvae_render_frame_bytes(26752, 26752, 1, 1, 0, 3) == 26752 * 26752 * 3          # 2^31 - 475 136 bytes
    assert lib.arvae_render_frame_bytes(30000, 30000, 1, 1, 2, 3) == -1 and b'2^31' in lib.arvae_last_error_string()
    assert lib.arvae_render_frame_bytes(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1, 2 ** 31 - 1, 3) == -1


def test_render_frames_host_checks(lib):
    """pure host code: every call returns before a launch (the pointers are never dereferenced)"""
    p = ctypes.c_void_p(64)

    def call(src=p, n_images=4, h=28, w=28, cells=p, n_frames=2, per_frame=6, nrow=8, padding=2, flags=5, out=p):
        return lib.arvae_render_frames(src, n_images, h, w, cells, n_frames, per_frame, nrow, padding, 1.0, flags, out, None)
    for null in ('src', 'cells', 'out'):
        assert call(**{null: None}) == -1 and b'null' in lib.arvae_last_error_string()
    for n_frames in (0, -3):
        assert call(n_frames=n_frames) == -1 and b'frames' in lib.arvae_last_error_string()
    assert call(n_images=0) == -1
    assert call(h=0) == -1 and call(w=-1) == -1 and call(per_frame=0) == -1 and call(nrow=0) == -1 and call(padding=-1) == -1
    assert call(flags=8) == -1 and b'flag' in lib.arvae_last_error_string()
    assert call(h=30000, w=30000, per_frame=1) == -1 and b'2^31' in lib.arvae_last_error_string()       # 2.7e9 bytes
    assert call(h=20000, w=20000, per_frame=6) == -1 and b'2^31' in lib.arvae_last_error_string()
    assert call(src=ctypes.c_void_p(66)) == -1 and b'aligned' in lib.arvae_last_error_string()


def test_wrapper_refusals():
    from arvae_amd import ops
    src = torch.zeros(4, 28, 28)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.render_frames(src, [[0, 1, 2, 3]])
    for bad in (4, -2):                                  # an index equal to n_images, and one below -1: refused before any launch
        with pytest.raises(ValueError, match=r'\[-1, 4\)'):
            ops.render_frames(src, np.array([[0, bad, 1]]))
        with pytest.raises(ValueError, match=r'\[-1, 4\)'):
            ops.render_frames(src, torch.tensor([[0, 1], [bad, -1]]))
    with pytest.raises(TypeError):
        ops.render_frames(src.double(), [[0]])
    with pytest.raises(ValueError):
        ops.render_frames(src, [0, 1])                   # cells are (frames, cells_per_frame)
    with pytest.raises(ValueError):
        ops.render_frames(src, [[0.5]])
    with pytest.raises(ValueError):
        ops.render_frames(torch.zeros(4, 3, 28, 28), [[0]])
    assert ops.render_geometry(28, 28, 6, 8, 2) == (32, 182) and ops.render_geometry(64, 64, 5, 8, 2) == (68, 332)
    assert ops.render_geometry(28, 28, 100, 10, 2) == (302, 302)


def test_restatement_equals_image_grid():
    """wherever nrow <= cells (image_grid always lays out nrow columns; make_grid min(nrow, cells)) the two grids agree"""
    from arvae_amd.logging_utils import image_grid
    rs = np.random.RandomState(5)
    checked = 0
    for (h, w) in fc.SHAPES[:3]:
        for n, nrow, padding in ((2, 1, 0), (5, 3, 1), (6, 3, 2), (9, 8, 2), (9, 3, 2), (8, 8, 2), (5, 5, 1)):
            for pad_value in (0.0, 1.0):
                images = rs.rand(n, h, w).astype(np.float32)
                want = image_grid(torch.from_numpy(images)[:, None], nrow, pad_value=pad_value, padding=padding).numpy()
                got = fc.grid(images, np.arange(n)[None], nrow, padding, np.float32(pad_value), 1)
                assert got.shape == (1,) + want.shape[1:] + (1,) and np.array_equal(got[0, :, :, 0], want[0])
                checked += 1
    assert checked == 42


def test_gif_and_png_round_trip(tmp_path):
    """grey RGB frames holding all 256 levels come back from the GIF bit for bit, with their count, size and timing"""
    from PIL import Image
    from arvae_amd import figures
    rs = np.random.RandomState(2)
    frames = np.repeat(rs.permutation(3 * 32 * 182).reshape(3, 32, 182, 1) % 256, 3, axis=3).astype(np.uint8)
    assert all(len(np.unique(f)) == 256 for f in frames)
    path = figures.write_gif(torch.from_numpy(frames), str(tmp_path / 'a.gif'), delay=70)
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.size == (182, 32) and im.info['duration'] == 70 and im.info['loop'] == 0
        for i in range(3):
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert('RGB')), frames[i]), i
    png = figures.write_png(frames[1], str(tmp_path / 'a.png'))
    with Image.open(png) as im:
        assert im.mode == 'RGB' and np.array_equal(np.asarray(im), frames[1])
    grey = figures.write_png(frames[:1, :, :, :1], str(tmp_path / 'g.png'))
    with Image.open(grey) as im:
        assert im.mode == 'L' and np.array_equal(np.asarray(im), frames[0, :, :, 0])
    with pytest.raises(TypeError):
        figures.write_png(frames[0].astype(np.float32), str(tmp_path / 'f.png'))


def test_cli_lists_the_switches(capsys):
    import train_image_vae
    with pytest.raises(SystemExit) as e:
        train_image_vae.run(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--gifs' in out and '--plots' in out and '--metrics' in out and '--digit_acc' in out
    assert 'scope' not in train_image_vae.__doc__


def test_trainer_has_the_figure_methods():
    import inspect
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    sig = {name: inspect.signature(getattr(ImageVAETrainer, name)).parameters
           for name in ('create_latent_gifs', 'plot_latent_interpolations', 'plot_latent_interpolations2d', 'plot_latent_reconstructions')}
    assert [(k, v.default) for k, v in sig['create_latent_gifs'].items()][1:] == [('sample_id', 9), ('num_points', 10), ('deterministic', False)]
    assert sig['plot_latent_interpolations']['attr_str'].default == 'slant'
    assert sig['plot_latent_interpolations']['sample_ids'].default == (5, 1, 30, 19, 23, 21, 17, 61, 9, 28)
    assert sig['plot_latent_interpolations2d']['sample_id'].default == 9
    for name in list(sig)[1:]:
        assert sig[name]['rounding'].default is True and sig[name]['deterministic'].default is False and sig[name]['num_points'].default == 10


# ---- the acceptance rule itself ---------------------------------------------------------------------------------------------------
def test_rule_on_the_quantiser_cases():
    for name, (src, logits, rounding, expect) in fc.quantiser_cases().items():
        cpu = fc.fp32_cpu_bytes(src, logits, rounding)
        assert np.array_equal(cpu, expect), (name, cpu.ravel(), expect.ravel())
        lo, hi = fc.interval(src, logits, rounding)
        assert np.all((lo <= cpu) & (cpu <= hi)), name
        if name.startswith('every_byte'):
            # built half a step from the quantiser's edges: fully determined.  The saturated ends are not the interval rule's to
            # decide (255 sigmoid(25) is below 255 in float64, so truncation gives 254 or 255): there the exact rule holds, a logit
            # from 20 on is 255 and one up to -20 is 0
            inner = np.abs(src) < 20.0
            assert np.array_equal(lo[inner], hi[inner]) and np.array_equal(lo[inner], expect[inner]) and inner.sum() >= 254, name


@pytest.mark.parametrize('rounding', [False, True])
def test_rule_on_the_random_case(rounding):
    src = fc.random_logits()
    assert src.shape == (64, 28, 28) and 2.9 < src.std() < 3.1
    lo, hi = fc.interval(src, True, rounding)
    cpu = fc.fp32_cpu_bytes(src, True, rounding)
    share = fc.undetermined_share(src, True, rounding)
    print(f'rounding {rounding}: {100 * share:.4f} % undetermined; bytes used {len(np.unique(cpu))}')
    assert share <= fc.MAX_UNDETERMINED
    assert np.all((lo <= cpu) & (cpu <= hi)) and np.all(hi - lo <= 1)
    assert len(np.unique(cpu)) >= 255                    # (truncation reaches 255 only where the sigmoid is exactly 1)


def test_rule_on_the_geometry_sources():
    """the geometry cases' sources are determined: both ends of the interval are the byte they were built from, and the pad bytes
    of the three pad values are what the fp32 arithmetic gives"""
    for shape in fc.SHAPES:
        for rounding in (False, True):
            v, b = fc.determined_images(shape, rounding, seed=11)
            lo, hi = fc.interval(v, False, rounding)
            assert np.array_equal(lo, b) and np.array_equal(hi, b) and np.array_equal(fc.fp32_cpu_bytes(v, False, rounding), b)
    assert [fc.pad_byte(p, False) for p in fc.PAD_VALUES] == [0, 127, 255]
    assert [fc.pad_byte(p, True) for p in fc.PAD_VALUES] == [0, 128, 255]

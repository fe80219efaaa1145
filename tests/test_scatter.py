"""Scatter figures without a GPU: the ABI of the new entry points and their host checks, the numpy restatement of
tests/scatter_cases.py by itself (layout, colour table, order of the blends), the library's layout of ticks and glyphs against
the restatement's, and the surface of the trainers and the two command lines."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import arvae_amd  # noqa: E402,F401
import scatter_cases as sc  # noqa: E402

NAMES = ('arvae_render_scatter_bytes', 'arvae_render_scatter')


@pytest.fixture(scope='module')
def lib():
    from arvae_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from arvae_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'arvae_hip.h')).read()
    assert re.search(r'#define ARVAE_ABI_VERSION 16\b', header) and _lib.ABI_VERSION == 16 and lib.arvae_abi_version() == 16
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NAMES:
        assert len(re.findall(r'\b' + name + r'\s*\(', code)) == 1, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert any(os.path.basename(s) == 'scatter.hip' for s in build.sources())
    for name, value in (('MAX_FIGURES', _lib.SCATTER_MAX_FIGURES), ('MAX_MARKS', _lib.SCATTER_MAX_MARKS), ('GLYPHS', len(sc.GLYPH_ORDER))):
        assert re.search(r'#define ARVAE_SCATTER_%s %d\b' % (name, value), header), name
    assert ctypes.sizeof(_lib.ScatterMark) == 8 and _lib.ScatterMark.figure.offset == 6
    assert (_lib.SCATTER_MAX_FIGURES, _lib.SCATTER_MAX_MARKS) == (sc.MAX_FIGURES, sc.MAX_MARKS)


def test_geometry_equals_the_restatement(lib):
    from arvae_amd import ops
    for width, height in ((485, 360), (226, 106), (141, 55), (1000, 700)):
        got = (ctypes.c_int32 * 6)()
        assert lib.arvae_render_scatter_bytes(width, height, 2, got) == width * height * 3
        g = sc.geometry(width, height)
        assert list(got) == [g[k] for k in ('px0', 'py0', 'pw', 'ph', 'bar_x', 'bar_w')]
        assert tuple(ops.scatter_geometry(width, height)) == tuple(got)
    assert tuple(ops.scatter_geometry()) == (57, 11, 360, 321, 429, 12)          # the default canvas, 485 x 360
    assert sc.geometry(**sc.SMALL)['pw'] == 101 and sc.geometry(**sc.SMALL)['ph'] == 67
    assert lib.arvae_render_scatter_bytes(485, 360, 2, None) == 485 * 360 * 3


def test_host_checks_refuse_before_any_launch(lib):
    """pure host code: every call returns ARVAE_E_INVALID with a message before a launch (the device pointers are never read)"""
    from arvae_amd._lib import ScatterMark
    p = ctypes.c_void_p(64)

    def render(points=p, values=p, f=1, n=10, limits=(-4, 4, -4, 4, 0, 1), width=485, height=360, radius=2, alpha=128, marks=(), n_marks=None,
               out=p, no_limits=False, no_marks=False):
        lim = (ctypes.c_float * (6 * max(f, 1)))(*(list(limits) * max(f, 1)))
        table = (ScatterMark * max(len(marks), 1))(*[ScatterMark(*m) for m in marks])
        return lib.arvae_render_scatter(points, values, f, n, None if no_limits else lim, width, height, radius, alpha,
                                        None if no_marks else table, len(marks) if n_marks is None else n_marks, out, None)

    def message():
        return lib.arvae_last_error_string()

    for null in (dict(points=None), dict(values=None), dict(out=None), dict(no_limits=True), dict(no_marks=True, n_marks=1)):
        assert render(**null) == -1 and b'null' in message(), null
    for f in (0, -1, 17):
        assert render(f=f) == -1 and b'figures' in message()
    assert render(n=-1) == -1 and render(n=2 ** 31) == -1 and b'points' in message()
    assert render(points=ctypes.c_void_p(68)) == -1 and b'aligned' in message()
    for limits in ((4, -4, -4, 4, 0, 1), (-4, 4, 1, 1, 0, 1), (float('nan'), 4, -4, 4, 0, 1), (-4, float('inf'), -4, 4, 0, 1),
                   (-3e38, 3e38, -4, 4, 0, 1)):
        assert render(limits=limits) == -1 and b'limits' in message(), limits
    for limits in ((-4, 4, -4, 4, 1, 0), (-4, 4, -4, 4, float('nan'), 1), (-4, 4, -4, 4, 0, float('inf'))):
        assert render(limits=limits) == -1 and b'vmin' in message(), limits
    for radius in (0, -1, 65):
        assert render(radius=radius) == -1 and b'radius' in message()
        assert lib.arvae_render_scatter_bytes(485, 360, radius, None) == -1
    for alpha in (-1, 257):
        assert render(alpha=alpha) == -1 and b'alpha' in message()
    # the canvas: too small for the margins (a plot area under 16 x 16), not positive, 32768 and more, 2^31 bytes and more
    for width, height in ((140, 360), (485, 54), (0, 360), (485, -1), (32768, 360), (485, 32768)):
        assert render(width=width, height=height) == -1, (width, height)
        assert lib.arvae_render_scatter_bytes(width, height, 2, None) == -1
    assert lib.arvae_render_scatter_bytes(140, 360, 2, None) == -1 and b'margins' in message()
    assert lib.arvae_render_scatter_bytes(141, 55, 2, None) == 141 * 55 * 3
    assert lib.arvae_render_scatter_bytes(32767, 32767, 2, None) == -1 and b'2^31' in message()
    # the table of marks: its capacity, and every entry of it
    assert render(n_marks=385) == -1 and b'capacity' in message()
    assert render(n_marks=-1) == -1
    assert render(marks=[(10, 10, 23, 0, -1)]) == -1 and b'glyph' in message()
    assert render(marks=[(10, 10, 3, 2, -1)]) == -1 and render(marks=[(10, 10, 21, 1, -1)]) == -1 and b'turned' in message()
    assert render(marks=[(10, 10, 3, 0, 1)]) == -1 and render(marks=[(10, 10, 3, 0, -2)]) == -1 and b'figure' in message()
    for x, y, glyph, rot in ((-1, 10, 3, 0), (10, -1, 3, 0), (481, 10, 3, 0), (10, 354, 3, 0), (479, 10, 3, 1), (10, 356, 3, 1),
                             (485, 10, 21, 0), (10, 357, 21, 0), (482, 10, 22, 0), (10, 360, 22, 0)):
        assert render(marks=[(480, 353, 3, 0, -1), (x, y, glyph, rot, -1)]) == -1 and b'canvas' in message(), (x, y, glyph, rot)


def test_wrappers_refuse():
    import torch
    from arvae_amd import ops
    pts, val = torch.zeros(2, 5, 2), torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.render_scatter(pts, val, (-4, 4), (-4, 4))
    with pytest.raises(TypeError):
        ops.render_scatter(pts.double(), val, (-4, 4), (-4, 4))
    for bad_pts, bad_val in ((pts[0], val), (pts, val[0]), (pts[:, :4], val), (pts[:1], val)):
        with pytest.raises(ValueError, match='points'):
            ops.render_scatter(bad_pts, bad_val, (-4, 4), (-4, 4))
    with pytest.raises(ValueError, match='figures'):
        ops.render_scatter(torch.zeros(17, 1, 2), torch.zeros(17, 1), (-4, 4), (-4, 4))
    for xlim in ((4, -4), (1, 1), (float('nan'), 1), (-4, 4, 5), [(-4, 4)] * 3):
        with pytest.raises(ValueError, match='xlim'):
            ops.render_scatter(pts, val, xlim, (-4, 4))
    with pytest.raises(ValueError, match='ylim'):
        ops.render_scatter(pts, val, (-4, 4), [(-4, 4), (2, 1)])
    for radius in (0, 1.5, -2):
        with pytest.raises(ValueError, match='radius'):
            ops.render_scatter(pts, val, (-4, 4), (-4, 4), radius=radius)
    for alpha in (-0.1, 1.5):
        with pytest.raises(ValueError, match='alpha'):
            ops.render_scatter(pts, val, (-4, 4), (-4, 4), alpha=alpha)
    for labels in (('a',), ('dimension: 0', 1), [('dimension: 0', 'dimension: 1')] * 3):
        with pytest.raises(ValueError, match='labels'):
            ops.render_scatter(pts, val, (-4, 4), (-4, 4), labels=labels)
    with pytest.raises(RuntimeError, match='margins'):
        ops.scatter_geometry(100, 100)
    with pytest.raises(ValueError, match='font'):
        ops.scatter_marks(ops.scatter_geometry(), (-4, 4), (-4, 4), (0, 1), ('dimension: 0', 'latent 1'))
    assert ops.SCATTER_FONT == sc.GLYPH_ORDER and set(sc.FONT) == set(sc.GLYPH_ORDER) == set('0123456789-.: dimension')


# ---- the layout: the library's marks are the restatement's cells -------------------------------------------------------------------------
LIMITS = [((-4.0, 4.0), (-4.0, 4.0), (0.0, 1.0)), ((-5.0, 5.0), (-5.0, 5.0), (0.25, 0.25)), ((-2.5, 3.0), (-1.0, 1.0), (0.25, 0.5)),
          ((-0.03, 0.07), (0.0, 26.0), (-1.0, 3.0)), ((-1234.0, 98765.0), (1e-4, 2e-4), (0.0, 1e9)), ((0.0, 101.0), (0.0, 67.0), (-0.5, 7.75))]


def test_ticks():
    assert sc.ticks(-4, 4) == [(-4.0, '-4'), (-2.0, '-2'), (0.0, '0'), (2.0, '2'), (4.0, '4')]
    assert [label for _, label in sc.ticks(-5, 5)] == ['-4', '-2', '0', '2', '4']
    assert [label for _, label in sc.ticks(0, 1)] == ['0.0', '0.2', '0.4', '0.6', '0.8', '1.0']
    assert [label for _, label in sc.ticks(-0.03, 0.07)] == ['-0.02', '0.00', '0.02', '0.04', '0.06']
    assert [label for _, label in sc.ticks(0, 26)] == ['0', '5', '10', '15', '20', '25']
    assert sc.ticks(0.25, 0.25) == [(0.25, '0.25')]
    for lo, hi in [pair for lim in LIMITS for pair in lim]:
        got = sc.ticks(lo, hi)
        assert 1 <= len(got) <= 7 and all(lo - 1e-6 * abs(lo) <= t <= hi + 1e-6 * abs(hi) for t, _ in got) and all(set(s) <= set('0123456789-.') for _, s in got)


@pytest.mark.parametrize('canvas', [(485, 360), (226, 106)])
def test_library_layout_is_the_restatements(canvas):
    from arvae_amd import ops
    g, geo = ops.scatter_geometry(*canvas), sc.geometry(*canvas)
    for xlim, ylim, vlim in LIMITS:
        for labels in (('dimension: 0', 'dimension: 1'), ('dimension: 31', 'dimension: 255')):
            assert [(round(t, 9), s) for t, s in ops.scatter_ticks(*xlim)] == [(round(t, 9), s) for t, s in sc.ticks(*xlim)]
            cells, xt, yt = sc.layout(geo, xlim, ylim, vlim, labels)
            want = {(x, y, sc.GLYPH_ORDER.index(ch), int(turned)) for x, y, ch, turned in cells if ch != ' '}
            want |= {(x, y, 21, 0) for x, y in xt} | {(x, y, 22, 0) for x, y in yt}
            assert ops.scatter_marks(g, xlim, ylim, vlim, labels) == want


def test_restatement_puts_things_where_the_geometry_says():
    """the frame, the colour bar and every glyph cell of the longest labels on both canvases"""
    for canvas in ((485, 360), (226, 106)):
        g = sc.geometry(*canvas)
        px0, py0, pw, ph, bar_x, bar_w = (g[k] for k in ('px0', 'py0', 'pw', 'ph', 'bar_x', 'bar_w'))
        assert px0 + pw + 12 == bar_x and bar_x + bar_w + 44 == canvas[0] and py0 + ph + 28 == canvas[1]
        labels = ('dimension: 255', 'dimension: 255')
        xlim, ylim, vlim = (-888.5, -887.5), (-100.5, -100.0), (-54321.0, 12345.0)          # labels of six characters on every axis
        img = sc.scatter(np.zeros((1, 0, 2), np.float32), np.zeros((1, 0), np.float32), xlim, ylim, vlim[0], vlim[1], width=canvas[0],
                         height=canvas[1], labels=labels)[0]
        assert img.shape == (canvas[1], canvas[0], 3)
        black = (img == 0).all(2)
        ring = np.zeros_like(black)
        ring[py0 - 1:py0 + ph + 1, px0 - 1:px0 + pw + 1] = True
        ring[py0:py0 + ph, px0:px0 + pw] = False
        assert black[ring].all() and (img[py0:py0 + ph, px0:px0 + pw] == 255).all()          # the frame, and an empty plot area
        bar = img[py0:py0 + ph, bar_x:bar_x + bar_w]
        assert (bar[0] == sc.VIRIDIS[255]).all() and (bar[-1] == sc.VIRIDIS[0]).all() and (bar == bar[:, :1]).all()
        assert black[py0 - 1, bar_x - 1:bar_x + bar_w + 1].all() and black[py0 - 1:py0 + ph + 1, bar_x + bar_w].all()
        cells, xt, yt = sc.layout(g, xlim, ylim, vlim, labels)
        assert all(max(len(s) for _, s in sc.ticks(*lim)) == sc.LABEL_CHARS for lim in (xlim, ylim, vlim))
        boxes = [sc.cell_box(x, y, turned) for x, y, _, turned in cells] + [(x, y, x + 1, y + 4) for x, y in xt] + [(x, y, x + 4, y + 1) for x, y in yt]
        assert len(boxes) <= sc.MAX_MARKS
        for x0, y0, x1, y1 in boxes:
            assert 0 <= x0 < x1 <= canvas[0] and 0 <= y0 < y1 <= canvas[1]
            inside_plot = x0 < px0 + pw + 1 and x1 > px0 - 1 and y0 < py0 + ph + 1 and y1 > py0 - 1
            inside_bar = x0 < bar_x + bar_w + 1 and x1 > bar_x - 1 and y0 < py0 + ph + 1 and y1 > py0 - 1
            assert not inside_plot and not inside_bar
        # all ink outside the two frames lies in those cells
        covered = np.zeros_like(black)
        for x0, y0, x1, y1 in boxes:
            covered[y0:y1, x0:x1] = True
        outside = np.ones_like(black)
        outside[py0 - 1:py0 + ph + 1, px0 - 1:px0 + pw + 1] = False
        outside[py0 - 1:py0 + ph + 1, bar_x - 1:bar_x + bar_w + 1] = False
        assert not (black & outside & ~covered).any() and (black & outside).sum() > 200
        assert ((img == 255).all(2) | black)[outside].all()


def test_colour_table_is_matplotlibs_viridis():
    cm = pytest.importorskip('matplotlib.cm')
    want = cm.viridis(np.arange(256), bytes=True)[:, :3]
    assert sc.VIRIDIS.shape == (256, 3) and np.array_equal(sc.VIRIDIS, want)


def test_quantisation_by_hand():
    pos, ok = sc.sixteenths([0.0, 101.0, 7.0, (3 + 0.5) / 16, -1e30, np.nan, np.inf, 3e38], 0.0, 101.0, 101)
    assert pos[:4].tolist() == [0, 1616, 112, 4] and ok.tolist() == [True] * 4 + [False] * 4
    assert sc.colour_index([0.0, 1.0, 0.5, -3.0, 7.0, 0.25], 0.0, 1.0).tolist() == [0, 255, 128, 0, 255, 64]
    assert sc.colour_index([0.1, 0.9], 0.5, 0.5).tolist() == [128, 128]
    assert sc.alpha256(0.5) == 128 and sc.alpha256(1.0) == 256 and sc.alpha256(0.3) == 77 and sc.alpha256(0.0) == 0
    assert sc.bounds([np.nan, 2.0, -np.inf, -1.0]) == (-1.0, 2.0) and sc.bounds([np.nan]) == (0.0, 0.0)


def test_later_point_is_on_top():
    """two overlapping points of different value: swapping them changes the pixels under both, and only those"""
    g = sc.geometry(**sc.SMALL)
    unit = ((0.0, float(g['pw'])), (0.0, float(g['ph'])))
    pts = np.array([[[40.0, 30.0], [43.0, 30.0]]], np.float32)
    val = np.array([[0.0, 1.0]], np.float32)
    for alpha in (0.5, 1.0, 0.3):
        a = sc.scatter(pts, val, *unit, 0.0, 1.0, radius=3, alpha=alpha, **sc.SMALL)[0]
        b = sc.scatter(pts[:, ::-1], val[:, ::-1], *unit, 0.0, 1.0, radius=3, alpha=alpha, **sc.SMALL)[0]
        differ = (a != b).any(2)
        yy, xx = np.mgrid[:a.shape[0], :a.shape[1]]
        cy = g['py0'] + g['ph'] - 30 - 0.5
        under = [(xx - (g['px0'] + x - 0.5)) ** 2 + (yy - cy) ** 2 <= 9 for x in (40.0, 43.0)]
        assert np.array_equal(differ, under[0] & under[1]) and differ.sum() > 5
        if alpha == 1.0:                                 # opaque: the overlap shows the later point's colour
            assert (a[differ] == sc.VIRIDIS[255]).all() and (b[differ] == sc.VIRIDIS[0]).all()
    # one marker over white at alpha 0.5: (255 * 256 * 128 + c * 256 * 128 + 128) >> 8, then rounded to a byte
    one = sc.scatter(pts[:, :1], val[:, :1], *unit, 0.0, 1.0, radius=1, alpha=0.5, **sc.SMALL)[0]
    c = sc.VIRIDIS[0].astype(np.int64)
    want = (((255 * 256 * 128 + c * 256 * 128 + 128) >> 8) + 128) >> 8
    hit = (one[g['py0']:g['py0'] + g['ph'], g['px0']:g['px0'] + g['pw']] != 255).any(2)
    assert hit.sum() == 4 and (one[g['py0']:g['py0'] + g['ph'], g['px0']:g['px0'] + g['pw']][hit] == want).all()


def test_case_table_reaches_what_it_is_there_for():
    cases = sc.raster_cases()
    clouds = [c for c in cases.values() if c['kind'] == 'cloud']
    assert {(c['n'], c['f']) for c in clouds} >= {(n, f) for n in sc.COUNTS for f in (1, 3)}
    assert {c['radius'] for c in clouds} == set(sc.RADII) and {c['alpha'] for c in clouds} == set(sc.ALPHAS)
    assert {c['small'] for c in clouds} == {True, False}
    assert {(c['radius'], c['alpha']) for c in clouds if c.get('spread')} == {(r, a) for r in sc.RADII for a in sc.ALPHAS}
    assert {c['kind'] for c in cases.values()} == {'cloud', 'corner', 'pile', 'limits', 'non_finite', 'flat', 'half_way'}
    g = sc.geometry(**sc.SMALL)
    # the corner case's disc centre lies on canvas pixel corner (64, 32): a corner of four 16 x 16 tiles
    pts, val, xlim, ylim, *_ = sc.case_inputs(cases['tile_corner'])
    x, _ = sc.sixteenths(pts[0, :, 0], *xlim, g['pw'])
    y, _ = sc.sixteenths(pts[0, :, 1], *ylim, g['ph'])
    assert (16 * g['px0'] + x[0]) == 16 * 64 and (16 * g['py0'] + 16 * g['ph'] - y[0]) == 16 * 32
    # the half-way case's products end in .5 exactly
    pts, val, xlim, ylim, *_ = sc.case_inputs(cases['half_way'])
    q = (pts[0].astype(np.float64) - 0.0) * 16.0
    assert np.all(q % 1.0 == 0.5) and len(q) > 100
    # the pile's 300 points share one position and not one value
    pts, val, *_ = sc.case_inputs(cases['one_pixel_300'])
    assert pts.shape == (1, 300, 2) and len(np.unique(pts.reshape(-1, 2), axis=0)) == 1 and len(np.unique(val)) > 50
    # the limits case has points that draw and points that do not on every side
    pts, val, xlim, ylim, vmin, vmax, look = sc.case_inputs(cases['limits'])
    img = sc.scatter(pts, val, xlim, ylim, vmin, vmax, **look)[0]
    plot = (img[g['py0']:g['py0'] + g['ph'], g['px0']:g['px0'] + g['pw']] != 255).any(2)
    assert plot[:, 0].any() and plot[:, -1].any() and plot[0].any() and plot[-1].any()
    for k in range(pts.shape[1]):                        # each point alone: those 4.2 and further out leave the plot area white
        alone = sc.scatter(pts[:, k:k + 1], val[:, k:k + 1], xlim, ylim, 0.0, 1.0, **look)[0]
        drew = (alone[g['py0']:g['py0'] + g['ph'], g['px0']:g['px0'] + g['pw']] != 255).any()
        assert drew == bool(np.abs(pts[0, k]).max() < 4.15), (k, pts[0, k])


# ---- trainers and command lines ---------------------------------------------------------------------------------------------------------
def _defaults(fn):
    return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]


def test_trainer_surface():
    from arvae_amd.image_vae_trainer import ImageVAETrainer
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    e = inspect._empty
    for cls in (MeasureVAETrainer, ImageVAETrainer):
        assert _defaults(cls.plot_data_dist)[1:6] == [('latent_codes', e), ('attributes', e), ('attr_str', e), ('dim1', 0), ('dim2', 1)]
    assert _defaults(MeasureVAETrainer.compute_latent_surface)[1:] == [('dim1', 0), ('dim2', 1), ('grid_res', 0.05), ('base_code', None),
                                                                       ('attr_list', None), ('chunk', 4096)]
    assert _defaults(MeasureVAETrainer.plot_latent_surface)[1:6] == [('attr_str', e), ('dim1', 0), ('dim2', 1), ('grid_res', 0.05), ('base_code', None)]


def test_cli_flags_parse_and_the_reference_surface_stays(capsys, monkeypatch):
    import train_image_vae
    import train_measure_vae
    for module, flags in ((train_measure_vae, ('--data_dist', '--surfaces')), (train_image_vae, ('--data_dist',))):
        with pytest.raises(SystemExit) as e:
            module.run(['--help'])
        assert e.value.code == 0
        out = capsys.readouterr().out
        assert all(flag in out for flag in flags)
        seen = {}
        monkeypatch.setattr(module, 'main', lambda args, seen=seen: seen.update(args=args))
        module.run(list(flags) + ['--test', '--rand', '3'])
        assert seen['args'] == ['--test', '--rand', '3']                     # the opt-in switches never reach the reference's flags
        assert module.with_data_dist is True and (module is train_image_vae or module.with_surfaces is True)
        module.run(['--test'])
        assert module.with_data_dist is False and (module is train_image_vae or module.with_surfaces is False)
        monkeypatch.undo()
    # main's parameters are the reference script's, in its order
    assert list(train_measure_vae.main.callback.__code__.co_varnames[:22]) == [
        'dataset_type', 'note_embedding_dim', 'metadata_embedding_dim', 'num_encoder_layers', 'encoder_hidden_size', 'encoder_dropout_prob',
        'latent_space_dim', 'num_decoder_layers', 'decoder_hidden_size', 'decoder_dropout_prob', 'has_metadata', 'batch_size', 'num_epochs',
        'lr', 'beta', 'capacity', 'gamma', 'delta', 'train', 'log', 'rand', 'reg_type']
    assert list(train_image_vae.main.callback.__code__.co_varnames[:13]) == [
        'dataset_type', 'batch_size', 'num_epochs', 'lr', 'beta', 'capacity', 'gamma', 'delta', 'dec_dist', 'train', 'log', 'rand', 'reg_type']
    assert sorted(p.name for p in train_measure_vae.main.params) == sorted(train_measure_vae.main.callback.__code__.co_varnames[:22])
    assert sorted(p.name for p in train_image_vae.main.params) == sorted(train_image_vae.main.callback.__code__.co_varnames[:13])

"""The scatter figures of csrc/scatter.hip restated in numpy, for tests/test_scatter.py and tests/test_scatter_gpu.py: the layout of a
canvas, the tick values and their labels, the 5 x 7 font, the two fp32 quantisations (coordinate -> sixteenths of a pixel, value ->
colour index), the disc coverage and the blending in input order in integers -- and the case table of the raster test.

Nothing here is taken from the library: the font is written out as pictures, the colour table as numbers (test_scatter.py holds
them to matplotlib's), the layout from include/arvae_hip.h's description."""
import math

import numpy as np

F32 = np.float32
FAR = F32(1048576.0)                                   # 2^20 sixteenths: positions outside (-FAR, FAR) draw nothing
MAX_FIGURES, MAX_MARKS, LABEL_CHARS = 16, 384, 6

# matplotlib's viridis at 256 levels, a colour as 0xBBGGRR
_VIRIDIS = [
    0x540144, 0x550244, 0x570344, 0x580545, 0x5a0645, 0x5b0845, 0x5c0946, 0x5e0b46,
    0x5f0c46, 0x610e46, 0x620f47, 0x631147, 0x651247, 0x661447, 0x671547, 0x691647,
    0x6a1847, 0x6b1948, 0x6c1a48, 0x6e1c48, 0x6f1d48, 0x701e48, 0x712048, 0x722148,
    0x732248, 0x742348, 0x752547, 0x762647, 0x772747, 0x782847, 0x792a47, 0x7a2b47,
    0x7b2c47, 0x7c2d46, 0x7c2f46, 0x7d3046, 0x7e3146, 0x7f3245, 0x7f3445, 0x803545,
    0x813645, 0x813744, 0x823944, 0x833a43, 0x833b43, 0x843c43, 0x843d42, 0x853e42,
    0x854042, 0x864141, 0x864241, 0x874340, 0x874440, 0x87453f, 0x88473f, 0x88483e,
    0x89493e, 0x894a3d, 0x894b3d, 0x894c3d, 0x8a4d3c, 0x8a4e3c, 0x8a503b, 0x8a513b,
    0x8b523a, 0x8b533a, 0x8b5439, 0x8b5539, 0x8b5638, 0x8c5738, 0x8c5837, 0x8c5937,
    0x8c5a36, 0x8c5b36, 0x8c5c35, 0x8c5d35, 0x8d5e34, 0x8d5f34, 0x8d6033, 0x8d6133,
    0x8d6232, 0x8d6332, 0x8d6431, 0x8d6531, 0x8d6631, 0x8d6730, 0x8d6830, 0x8d692f,
    0x8d6a2f, 0x8e6b2e, 0x8e6c2e, 0x8e6d2e, 0x8e6e2d, 0x8e6f2d, 0x8e702c, 0x8e712c,
    0x8e722c, 0x8e732b, 0x8e742b, 0x8e752a, 0x8e762a, 0x8e772a, 0x8e7829, 0x8e7929,
    0x8e7a28, 0x8e7a28, 0x8e7b28, 0x8e7c27, 0x8e7d27, 0x8e7e27, 0x8e7f26, 0x8e8026,
    0x8e8126, 0x8e8225, 0x8d8325, 0x8d8424, 0x8d8524, 0x8d8624, 0x8d8723, 0x8d8823,
    0x8d8923, 0x8d8922, 0x8d8a22, 0x8d8b22, 0x8d8c21, 0x8c8d21, 0x8c8e21, 0x8c8f20,
    0x8c9020, 0x8c9120, 0x8c921f, 0x8b931f, 0x8b941f, 0x8b951f, 0x8b961f, 0x8a971e,
    0x8a981e, 0x8a991e, 0x8a991e, 0x899a1e, 0x899b1e, 0x899c1e, 0x889d1e, 0x889e1e,
    0x889f1e, 0x87a01e, 0x87a11f, 0x86a21f, 0x86a31f, 0x85a420, 0x85a520, 0x85a621,
    0x84a721, 0x84a722, 0x83a823, 0x82a923, 0x82aa24, 0x81ab25, 0x81ac26, 0x80ad27,
    0x7fae28, 0x7faf29, 0x7eb02a, 0x7db12b, 0x7db12c, 0x7cb22e, 0x7bb32f, 0x7ab430,
    0x7ab532, 0x79b633, 0x78b735, 0x77b836, 0x76b938, 0x76b939, 0x75ba3b, 0x74bb3d,
    0x73bc3e, 0x72bd40, 0x71be42, 0x70be44, 0x6fbf45, 0x6ec047, 0x6dc149, 0x6cc24b,
    0x6bc24d, 0x69c34f, 0x68c451, 0x67c553, 0x66c655, 0x65c657, 0x64c759, 0x62c85b,
    0x61c95e, 0x60c960, 0x5fca62, 0x5dcb64, 0x5ccc67, 0x5bcc69, 0x59cd6b, 0x58ce6d,
    0x56ce70, 0x55cf72, 0x54d074, 0x52d077, 0x51d179, 0x4fd27c, 0x4ed27e, 0x4cd381,
    0x4bd383, 0x49d486, 0x47d588, 0x46d58b, 0x44d68d, 0x43d690, 0x41d792, 0x3fd795,
    0x3ed897, 0x3cd89a, 0x3ad99d, 0x38d99f, 0x37daa2, 0x35daa5, 0x33dba7, 0x32dbaa,
    0x30dcad, 0x2edcaf, 0x2cddb2, 0x2bddb5, 0x29ddb7, 0x27deba, 0x26debd, 0x24dfbf,
    0x22dfc2, 0x21dfc5, 0x1fe0c7, 0x1ee0ca, 0x1de0cd, 0x1ce1cf, 0x1be1d2, 0x1ae1d4,
    0x19e2d7, 0x18e2da, 0x18e2dc, 0x18e3df, 0x18e3e1, 0x18e3e4, 0x19e4e7, 0x19e4e9,
    0x1ae4ec, 0x1be5ee, 0x1ce5f1, 0x1ee5f3, 0x1fe6f6, 0x21e6f8, 0x22e6fa, 0x24e7fd,
]
VIRIDIS = np.array([[c & 255, (c >> 8) & 255, c >> 16] for c in _VIRIDIS], np.uint8)          # (256, 3) RGB

FONT = {
    '0': ['.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'],
    '1': ['..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'],
    '2': ['.###.', '#...#', '....#', '...#.', '..#..', '.#...', '#####'],
    '3': ['.###.', '#...#', '....#', '..##.', '....#', '#...#', '.###.'],
    '4': ['...#.', '..##.', '.#.#.', '#..#.', '#####', '...#.', '...#.'],
    '5': ['#####', '#....', '####.', '....#', '....#', '#...#', '.###.'],
    '6': ['.###.', '#....', '#....', '####.', '#...#', '#...#', '.###.'],
    '7': ['#####', '....#', '...#.', '..#..', '..#..', '..#..', '..#..'],
    '8': ['.###.', '#...#', '#...#', '.###.', '#...#', '#...#', '.###.'],
    '9': ['.###.', '#...#', '#...#', '.####', '....#', '....#', '.###.'],
    '-': ['.....', '.....', '.....', '.###.', '.....', '.....', '.....'],
    '.': ['.....', '.....', '.....', '.....', '.....', '.##..', '.##..'],
    ':': ['.....', '.##..', '.##..', '.....', '.##..', '.##..', '.....'],
    ' ': ['.....', '.....', '.....', '.....', '.....', '.....', '.....'],
    'd': ['....#', '....#', '.####', '#...#', '#...#', '#...#', '.####'],
    'i': ['..#..', '.....', '.##..', '..#..', '..#..', '..#..', '.###.'],
    'm': ['.....', '.....', '##.#.', '#.#.#', '#.#.#', '#.#.#', '#.#.#'],
    'e': ['.....', '.....', '.###.', '#...#', '#####', '#....', '.###.'],
    'n': ['.....', '.....', '#.##.', '##..#', '#...#', '#...#', '#...#'],
    's': ['.....', '.....', '.####', '#....', '.###.', '....#', '####.'],
    'o': ['.....', '.....', '.###.', '#...#', '#...#', '#...#', '.###.'],
}
GLYPH_ORDER = '0123456789-.: dimenso'                  # a glyph's number in arvae_scatter_mark_t


def geometry(width=485, height=360):
    """the plot area's first pixel and extent, the colour bar's first column and width"""
    pw, ph = width - 125, height - 39
    return dict(px0=57, py0=11, pw=pw, ph=ph, bar_x=57 + pw + 12, bar_w=12)


def ticks(lo, hi, most=6):
    """[(value, label)]: the multiples of the smallest step 1, 2, 5 x 10^k with at most most + 1 of them between lo and hi"""
    lo, hi = float(lo), float(hi)
    if lo == hi:
        return [(lo, '%.2f' % lo)]
    raw = (hi - lo) / most
    k = math.floor(math.log10(raw))
    m = next(m for m in (1, 2, 5, 10) if m * 10.0 ** k >= raw)
    step = m * 10.0 ** k
    decimals = max(0, -k - 1) if m == 10 else max(0, -k)
    out = []
    for i in range(math.ceil(lo / step - 1e-9), math.floor(hi / step + 1e-9) + 1):
        label = '%.*f' % (decimals, i * step)
        if float(label) == 0:
            label = label.replace('-', '')
        out.append((i * step, label))
    return out


def tick_pixel(t, lo, hi, extent):
    if lo == hi:
        return (extent - 1) // 2
    return min(extent - 1, max(0, int(math.floor((t - lo) / (hi - lo) * (extent - 1) + 0.5))))


def text_cells(s, x, y, turned=False):
    """[(x, y, character)] of the cells of a string: upright from (x, y) to the right, 6 pixels a character; turned a quarter to the
    left from the cell whose BOTTOM row is y upwards"""
    return [((x, y - 6 * i - 4, ch) if turned else (x + 6 * i, y, ch)) for i, ch in enumerate(s)]


def layout(g, xlim, ylim, vlim, labels):
    """(glyph cells [(x, y, character, turned)], x tick marks [(x, y)] of 1 x 4, y tick marks [(x, y)] of 4 x 1) of one figure"""
    cells, xt, yt = [], [], []
    for t, label in ticks(*xlim):
        cx = g['px0'] + tick_pixel(t, xlim[0], xlim[1], g['pw'])
        xt.append((cx, g['py0'] + g['ph'] + 1))
        if len(label) <= LABEL_CHARS:
            cells += [c + (False,) for c in text_cells(label, cx - (6 * len(label) - 1) // 2, g['py0'] + g['ph'] + 7)]
    for t, label in ticks(*ylim):
        cy = g['py0'] + g['ph'] - 1 - tick_pixel(t, ylim[0], ylim[1], g['ph'])
        yt.append((g['px0'] - 5, cy))
        if len(label) <= LABEL_CHARS:
            cells += [c + (False,) for c in text_cells(label, g['px0'] - 7 - (6 * len(label) - 1), cy - 3)]
    for t, label in ticks(*vlim):
        cy = g['py0'] + g['ph'] - 1 - tick_pixel(t, vlim[0], vlim[1], g['ph'])
        yt.append((g['bar_x'] + g['bar_w'] + 1, cy))
        if len(label) <= LABEL_CHARS:
            cells += [c + (False,) for c in text_cells(label, g['bar_x'] + g['bar_w'] + 7, cy - 3)]
    cells += [c + (False,) for c in text_cells(labels[0], g['px0'] + g['pw'] // 2 - (6 * len(labels[0]) - 1) // 2, g['py0'] + g['ph'] + 18)]
    cells += [c + (True,) for c in text_cells(labels[1], 3, g['py0'] + g['ph'] // 2 + (6 * len(labels[1]) - 1) // 2, turned=True)]
    return cells, xt, yt


def cell_box(x, y, turned):
    """(x0, y0, x1, y1), exclusive, of a glyph's cell"""
    return (x, y, x + 7, y + 5) if turned else (x, y, x + 5, y + 7)


def sixteenths(coord, lo, hi, extent):
    """(position in sixteenths of a pixel from the axis's start as int64, valid): fp32 subtract, multiply, add, each rounded"""
    coord = np.asarray(coord, F32)
    k = F32(16 * extent) / (F32(hi) - F32(lo))
    with np.errstate(invalid='ignore', over='ignore'):
        q = (coord - F32(lo)) * k
        valid = (q > -FAR) & (q < FAR)
        pos = np.floor(np.where(valid, q, F32(0)) + F32(0.5)).astype(np.int64)
    return pos, valid


def colour_index(values, vmin, vmax):
    values = np.asarray(values, F32)
    den = F32(vmax) - F32(vmin)
    if den == 0:
        return np.full(values.shape, 128, np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        c = (values - F32(vmin)) / den
        c = np.fmin(np.fmax(c, F32(0)), F32(1))
        return np.floor(np.where(np.isfinite(c), c, F32(0)) * F32(255) + F32(0.5)).astype(np.int64)


def bounds(values):
    """the finite minimum and maximum of a figure's values, (0, 0) without a finite one"""
    v = np.asarray(values, F32)
    v = v[np.isfinite(v)]
    return (float(v.min()), float(v.max())) if v.size else (0.0, 0.0)


def alpha256(alpha):
    return int(math.floor(alpha * 256 + 0.5))


def figure(points, values, xlim, ylim, vmin=None, vmax=None, width=485, height=360, radius=2, alpha=0.5,
           labels=('dimension: 0', 'dimension: 1')):
    """one figure, (height, width, 3) uint8"""
    points, values = np.asarray(points, F32).reshape(-1, 2), np.asarray(values, F32).reshape(-1)
    lo, hi = bounds(values)
    vmin, vmax = (lo if vmin is None else vmin), (hi if vmax is None else vmax)
    xlim, ylim = tuple(float(F32(v)) for v in xlim), tuple(float(F32(v)) for v in ylim)       # the limits are fp32 numbers
    g = geometry(width, height)
    px0, py0, pw, ph, bar_x, bar_w = (g[k] for k in ('px0', 'py0', 'pw', 'ph', 'bar_x', 'bar_w'))
    img = np.full((height, width, 3), 255, np.uint8)
    cells, xt, yt = layout(g, xlim, ylim, (float(F32(vmin)), float(F32(vmax))), labels)
    for x, y, ch, turned in cells:
        for r, line in enumerate(FONT[ch]):
            for c, ink in enumerate(line):
                if ink == '#':
                    if turned:
                        img[y + 4 - c, x + r] = 0
                    else:
                        img[y + r, x + c] = 0
    for x, y in xt:
        img[y:y + 4, x] = 0
    for x, y in yt:
        img[y, x:x + 4] = 0
    # the two frames cover whatever a mark put there; then the bar, then the plot area
    img[py0 - 1:py0 + ph + 1, px0 - 1:px0 + pw + 1] = 0
    img[py0 - 1:py0 + ph + 1, bar_x - 1:bar_x + bar_w + 1] = 0
    rows = np.arange(ph)
    img[py0:py0 + ph, bar_x:bar_x + bar_w] = VIRIDIS[((ph - 1 - rows) * 255 + (ph - 1) // 2) // (ph - 1)][:, None, :]
    plot = np.full((ph, pw, 3), 255 * 256, np.int64)
    xs, okx = sixteenths(points[:, 0], xlim[0], xlim[1], pw)
    ys, oky = sixteenths(points[:, 1], ylim[0], ylim[1], ph)
    ys = 16 * ph - ys
    draw = okx & oky & np.isfinite(values)
    colours = VIRIDIS[colour_index(np.where(draw, values, F32(vmin)), vmin, vmax)].astype(np.int64)
    a, r16 = alpha256(alpha), 16 * radius
    for i in np.flatnonzero(draw):                       # in the order of the input
        x, y = int(xs[i]), int(ys[i])
        i0, i1 = max(0, (x - r16 - 8) // 16), min(pw, (x + r16 - 8) // 16 + 1)
        j0, j1 = max(0, (y - r16 - 8) // 16), min(ph, (y + r16 - 8) // 16 + 1)
        if i0 >= i1 or j0 >= j1:
            continue
        dx = 16 * np.arange(i0, i1) + 8 - x
        dy = 16 * np.arange(j0, j1) + 8 - y
        inside = dx[None, :] ** 2 + dy[:, None] ** 2 <= r16 * r16
        part = plot[j0:j1, i0:i1]
        part[inside] = (part[inside] * (256 - a) + colours[i] * 256 * a + 128) >> 8
    img[py0:py0 + ph, px0:px0 + pw] = ((plot + 128) >> 8).astype(np.uint8)
    return img


def scatter(points, values, xlim, ylim, vmin=None, vmax=None, **look):
    """(F, N, 2) points and (F, N) values -> (F, height, width, 3); xlim, ylim, vmin, vmax and labels for all figures or one each"""
    points, values = np.asarray(points, F32), np.asarray(values, F32)
    f = values.shape[0]

    def each(v, i, pair):
        a = np.asarray(v)
        return v if a.ndim == (1 if pair else 0) else v[i]
    labels = look.pop('labels', ('dimension: 0', 'dimension: 1'))
    frames = []
    for i in range(f):
        lab = labels if isinstance(labels[0], str) else labels[i]
        frames.append(figure(points[i], values[i], each(xlim, i, True), each(ylim, i, True), None if vmin is None else each(vmin, i, False),
                             None if vmax is None else each(vmax, i, False), labels=lab, **look))
    return np.stack(frames)


# ---- the case table of the raster test -----------------------------------------------------------------------------------------------
SMALL = dict(width=226, height=106)                    # a plot area of 101 x 67: neither a multiple of the 16-pixel tile
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)       # the wavefront's and the chunk's edges of the ordered compaction
RADII = (1, 2, 5)
ALPHAS = (0.5, 1.0, 0.3)


def raster_cases():
    """name -> keywords of case_inputs"""
    cases = {}
    for k, n in enumerate(COUNTS):                       # every count at both figure counts; canvas, radius and alpha go round
        for f in (1, 3):
            j = k + (f == 3)
            cases[f'n{n}_f{f}'] = dict(kind='cloud', n=n, f=f, small=(j % 2 == 0), radius=RADII[j % 3], alpha=ALPHAS[(j // 2) % 3])
    for radius in RADII:                                 # every radius with every alpha on the small canvas, points overlapping
        for alpha in ALPHAS:
            cases[f'dense_r{radius}_a{alpha}'] = dict(kind='cloud', n=257, f=1, small=True, radius=radius, alpha=alpha, spread=0.15)
    cases['default_canvas_f3'] = dict(kind='cloud', n=1000, f=3, small=False, radius=2, alpha=0.5)
    cases['tile_corner'] = dict(kind='corner', radius=5, alpha=0.5)
    cases['one_pixel_300'] = dict(kind='pile', n=300, radius=2, alpha=0.3)
    cases['limits'] = dict(kind='limits', radius=2, alpha=0.5)
    cases['non_finite'] = dict(kind='non_finite', radius=2, alpha=0.5)
    cases['vmin_equals_vmax_given'] = dict(kind='flat', given=True, radius=2, alpha=0.5)
    cases['vmin_equals_vmax_found'] = dict(kind='flat', given=False, radius=2, alpha=1.0)
    cases['half_way'] = dict(kind='half_way', radius=1, alpha=1.0)
    return cases


def case_inputs(case):
    """-> (points (F, N, 2), values (F, N), xlim, ylim, vmin, vmax, look)"""
    kind = case['kind']
    look = dict(radius=case['radius'], alpha=case['alpha'])
    if kind == 'cloud':
        f, n = case['f'], case['n']
        rng = np.random.RandomState(1000 * f + n + case['radius'])
        if case['small']:
            look.update(SMALL)
        points = (rng.randn(f, n, 2) * case.get('spread', 1.6)).astype(F32)
        values = rng.rand(f, n).astype(F32)
        if f == 1:
            return points, values, (-4.0, 4.0), (-4.0, 4.0), None, None, look
        look['labels'] = [('dimension: %d' % i, 'dimension: %d' % (31 - i)) for i in range(f)]
        xlim = [(-4.0, 4.0), (-2.5, 3.0), (-5.0, 5.0)]
        ylim = [(-4.0, 4.0), (-1.0, 1.0), (-0.03, 0.07)]
        return points, values, xlim, ylim, [0.0, 0.25, -1.0], [1.0, 0.5, 3.0], look
    look.update(SMALL)
    pw, ph = geometry(**SMALL)['pw'], geometry(**SMALL)['ph']
    unit = ((0.0, float(pw)), (0.0, float(ph)))          # a pixel a unit: k = 16 exactly
    if kind == 'corner':                                 # canvas pixel corner (64, 32) = plot corner (7, 21): four tiles meet there
        points = np.array([[[7.0, ph - 21.0]]], F32)
        return points, np.array([[0.7]], F32), unit[0], unit[1], 0.0, 1.0, look
    if kind == 'pile':                                   # one pixel, values going up and down: the order of 300 blends matters
        n = case['n']
        points = np.tile(np.array([50.5, 30.5], F32), (1, n, 1))
        values = ((np.arange(n) * 37) % 101 / 100.0).astype(F32)[None]
        return points, values, unit[0], unit[1], 0.0, 1.0, look
    if kind == 'limits':                                 # on, just inside and just outside each limit, and a radius and more outside
        lo, hi = F32(-4.0), F32(4.0)
        edge = [lo, np.nextafter(lo, F32(9)), np.nextafter(lo, F32(-9)), hi, np.nextafter(hi, F32(9)), np.nextafter(hi, F32(-9)),
                F32(-4.1), F32(-4.2), F32(4.1), F32(4.2), F32(-1e30), F32(1e30), F32(3e38)]
        pts = [(e, F32(0.5 * i - 3)) for i, e in enumerate(edge)] + [(F32(0.5 * i - 3), e) for i, e in enumerate(edge)]
        pts += [(a, b) for a in (lo, hi) for b in (lo, hi)]
        points = np.array(pts, F32)[None]
        values = np.linspace(0, 1, points.shape[1]).astype(F32)[None]
        return points, values, (-4.0, 4.0), (-4.0, 4.0), None, None, look
    if kind == 'non_finite':
        bad = [np.nan, np.inf, -np.inf]
        pts = [(b, 0.0) for b in bad] + [(0.0, b) for b in bad] + [(1.0, 1.0)] * 3 + [(-1.0, 0.5), (2.0, -2.0)]
        vals = [0.1] * 6 + bad + [0.2, 0.9]
        return np.array(pts, F32)[None], np.array(vals, F32)[None], (-4.0, 4.0), (-4.0, 4.0), None, None, look
    if kind == 'flat':
        rng = np.random.RandomState(5)
        points = rng.randn(1, 40, 2).astype(F32)
        if case['given']:
            return points, rng.rand(1, 40).astype(F32), (-4.0, 4.0), (-4.0, 4.0), 0.5, 0.5, look
        return points, np.full((1, 40), 0.25, F32), (-4.0, 4.0), (-4.0, 4.0), None, None, look
    if kind == 'half_way':                               # (n + 0.5) / 16 pixels: the product is n + 0.5 exactly and rounds up
        n = np.arange(0, 16 * 60, 7)
        points = np.stack([(n + 0.5) / 16.0 + 20.0, (n % 29 + 0.5) / 16.0 + 10.0], 1).astype(F32)[None]
        values = (n % 13 / 12.0).astype(F32)[None]
        return points, values, unit[0], unit[1], 0.0, 1.0, look
    raise KeyError(kind)

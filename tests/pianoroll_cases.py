"""What the piano-roll tests (test_pianoroll.py on the CPU, test_pianoroll_gpu.py on the GPU) share: the oracle and the case tables.

The reference's figure code needs music21, pretty_midi and pypianoroll, which cannot be run here, so no golden is recorded from it.
The oracle is a restatement in Python, written from the reference's source:
  * m21_elements / m21_sequence: tensor_to_m21score and concatenate_scores (data/dataloaders/bar_dataset.py:224-268) with
    fractions.Fraction quarter lengths, TICK_VALUES and compute_tick_durations as in bar_dataset_helpers.py.  One choice is this
    project's: the vocabulary's `None` entry is silence (build_measure_tables' is_note), where the reference would hand None to
    music21's Note constructor;
  * events: the same in integers, per tick, in twelfths of a quarter note -- what arvae_measure_notes must equal;
  * pianoroll: the raster of arvae_render_pianoroll, painted layer by layer from those events (the kernel decides pixel by pixel).
    The look is this project's own: the reference's comes out of matplotlib and pypianoroll.
"""
import itertools
from fractions import Fraction

import numpy as np

from arvae_amd import synthetic as syn

TICK_START = (0, 3, 4, 6, 8, 9)
DARK = np.array([8, 48, 107])                            # matplotlib's darkest "Blues"


def tick_twelfth(t):
    return 12 * (t // 6) + TICK_START[t % 6]


def vocabulary():
    """(index2note, note2index, midi, is_note, slur, V) of the synthetic vocabulary: '__', START, END, rest, None, G3 .. C6"""
    i2n, n2i = syn.measure_vocabulary()
    midi, is_note, _ = syn.measure_tables()
    return i2n, n2i, midi, is_note, n2i['__'], len(i2n)


# ---- the reference's conversion, in fractions ---------------------------------------------------------------------------------------
TICK_VALUES = [Fraction(0), Fraction(1, 4), Fraction(1, 3), Fraction(1, 2), Fraction(2, 3), Fraction(3, 4)]
TICK_DURATIONS = [b - a for a, b in zip(TICK_VALUES, TICK_VALUES[1:] + [Fraction(1)])]


def m21_elements(row, index2note, slur):
    """one measure -> [(MIDI pitch or 0 for a rest, quarter length)] in the order the part receives them"""
    out, dur, cur = [], Fraction(0), 0                   # the pending element starts out as a rest without duration
    for tick, x in enumerate(row):
        if x != slur:
            if dur > 0:
                out.append((cur, dur))
            dur = TICK_DURATIONS[tick % 6]
            sym = index2note[int(x)]
            cur = 0 if sym in ('rest', '__', 'START', 'END', None) else syn.name_to_midi(sym)
        else:
            dur += TICK_DURATIONS[tick % 6]
    out.append((cur, dur))
    return out


def m21_sequence(rows, index2note, slur):
    """measures -> [(offset, quarter length, pitch or 0)]: every measure's elements one after the other from 4 k on"""
    out = []
    for k, row in enumerate(rows):
        at = Fraction(4 * k)
        for pitch, dur in m21_elements(row, index2note, slur):
            out.append((at, dur, pitch))
            at += dur
    return out


# ---- the events in integers -----------------------------------------------------------------------------------------------------------
def events(score, midi, is_note, slur):
    """(M, T) indices -> (M, T, 3) int32 [pitch sounding (0: silence), first tick of the element (-1: leading slurs), length in
    twelfths on the element's first tick (0 elsewhere)]"""
    score = np.asarray(score)
    m, t = score.shape
    out = np.zeros((m, t, 3), np.int32)
    for r in range(m):
        start, pitch = -1, 0
        for i in range(t):
            x = int(score[r, i])
            if x != slur:
                if start >= 0:
                    out[r, start, 2] = tick_twelfth(i) - tick_twelfth(start)
                start = i
                pitch = int(midi[x]) if 0 <= x < len(midi) and is_note[x] else 0
            out[r, i, 0], out[r, i, 1] = pitch, start
        if start >= 0:
            out[r, start, 2] = 2 * t - tick_twelfth(start)
    return out


def sounding(ev):
    """(M, T, 3) events -> [(onset, length, pitch)] in twelfths from the start of the first measure"""
    m, t, _ = ev.shape
    return [(r * 2 * t + tick_twelfth(i), int(ev[r, i, 2]), int(ev[r, i, 0])) for r in range(m) for i in range(t)
            if ev[r, i, 2] > 0 and ev[r, i, 0] > 0]


def corner_rows(t=24):
    """name -> one measure of t ticks"""
    _, n2i, _, _, slur, v = vocabulary()
    g4, a4, c6, g3 = n2i['G4'], n2i['A4'], n2i['C6'], n2i['G3']
    rows = {'all slurs': [slur] * t,
            'slurs then a note': [slur] * (t // 2) + [g4] + [slur] * (t - t // 2 - 1),
            'every tick': [(g3 + i) % v if (g3 + i) % v != slur else g4 for i in range(t)],
            'note on the last tick': [a4] + [slur] * (t - 2) + [c6],
            'token -1 and V': [g4, slur, -1, slur, v, slur] + [slur] * (t - 6)}
    for sym in ('rest', 'START', 'END', None):           # in the middle of a held note
        rows[f'{sym} inside a note'] = [g4] + [slur] * (t // 2 - 1) + [n2i[sym]] + [slur] * (t - t // 2 - 1)
    return {k: np.array(r, np.int64) for k, r in rows.items()}


def random_measures(m, t, seed, p_slur=0.6):
    """(m, t) indices: P(slur) = p_slur, the other symbols uniform"""
    rs = np.random.RandomState(seed)
    _, _, _, _, slur, v = vocabulary()
    other = rs.randint(0, v - 1, (m, t))
    other = other + (other >= slur)
    return np.where(rs.random_sample((m, t)) < p_slur, slur, other).astype(np.int64)


def measures(m, t, seed):
    """the corner rows first (as many as fit), then random ones"""
    rows = np.stack(list(corner_rows(t).values()))
    return np.concatenate([rows, random_measures(max(m - len(rows), 0), t, seed)])[:m] if m > 1 else random_measures(1, t, seed, 0.4)


# ---- the raster -----------------------------------------------------------------------------------------------------------------------
def default_mark(px_per_twelfth):
    return max(1, 12 * px_per_twelfth // 20)


def geometry(k, t, with_panel, pitch_lo=55, pitch_hi=84, px_per_twelfth=2, px_per_pitch=4, panel_cell=12, gap=8):
    """-> (H, roll width, W)"""
    roll_w = k * (t // 6) * 12 * px_per_twelfth
    return (pitch_hi - pitch_lo + 1) * px_per_pitch, roll_w, roll_w + (gap + k * panel_cell if with_panel else 0)


def value_bounds(values, vmin=None, vmax=None):
    v = np.asarray(values, np.float32)
    finite = v[np.isfinite(v)]
    lo, hi = (float(finite.min()), float(finite.max())) if finite.size else (0.0, 0.0)
    return np.float32(lo if vmin is None else vmin), np.float32(hi if vmax is None else vmax)


def disc_row(value, vmin, vmax, h):
    """fp32, every operation rounded by itself"""
    value, vmin, vmax = np.float32(value), np.float32(vmin), np.float32(vmax)
    with np.errstate(over='ignore', invalid='ignore'):
        c = np.float32(0.5) if vmax == vmin else (value - vmin) / (vmax - vmin)
        c = min(max(c, np.float32(0.0)), np.float32(1.0))
        return h - 1 - int(np.floor(c * np.float32(h - 1) + np.float32(0.5)))


def pianoroll(score, midi, is_note, slur, values=None, vmin=None, vmax=None, pitch_lo=55, pitch_hi=84, px_per_twelfth=2, px_per_pitch=4,
              mark=None, panel_cell=12, gap=8, dot_radius=3):
    """(F, K, T) indices -> (F, H, W, 3) uint8"""
    score = np.asarray(score)
    f, k, t = score.shape
    ppt, ppp = px_per_twelfth, px_per_pitch
    mark = default_mark(ppt) if mark is None else mark
    h, roll_w, w = geometry(k, t, values is not None, pitch_lo, pitch_hi, ppt, ppp, panel_cell, gap)
    measure_w = roll_w // k
    ev = events(score.reshape(f * k, t), midi, is_note, slur).reshape(f, k, t, 3)

    def rows(p):
        return slice((pitch_hi - p) * ppp, (pitch_hi - p + 1) * ppp) if pitch_lo <= p <= pitch_hi else slice(0, 0)

    shade = np.zeros((f, h, roll_w), np.int64)
    for p in range(pitch_lo, pitch_hi + 1):
        if p % 2 == 0:
            shade[:, rows(p)] = 30
    shade[:, :, ::12 * ppt] = 50
    shade[:, :, ::measure_w] = 100
    spans = [(a, b * measure_w + tick_twelfth(c) * ppt, int(ev[a, b, c, 2]) * ppt, int(ev[a, b, c, 0]))
             for a in range(f) for b in range(k) for c in range(t) if ev[a, b, c, 2] > 0 and ev[a, b, c, 0] > 0]
    for a, x0, width, p in spans:
        shade[a, rows(p), x0:x0 + width] = 90
    for a, x0, width, p in spans:
        for q in (p - 1, p, p + 1):
            shade[a, rows(q), x0:x0 + min(mark, width)] = 127
    out = np.full((f, h, w, 3), 255, np.uint8)
    out[:, :, :roll_w] = 255 - (shade[..., None] * (255 - DARK) + 63) // 127
    if values is not None:
        lo, hi = value_bounds(values, vmin, vmax)
        for a in range(f):
            for b in range(k):
                if not np.isfinite(values[a][b]):
                    continue
                cell = roll_w + gap + b * panel_cell
                row, col = disc_row(values[a][b], lo, hi, h), cell + panel_cell // 2
                for dy in range(-dot_radius, dot_radius + 1):
                    for dx in range(-dot_radius, dot_radius + 1):
                        if dx * dx + dy * dy <= dot_radius * dot_radius and 0 <= row + dy < h and cell <= col + dx < cell + panel_cell:
                            out[a, row + dy, col + dx] = 0
    return out


# ---- raster cases ---------------------------------------------------------------------------------------------------------------------
PX_PER_TWELFTH, PX_PER_PITCH, MEASURES, FIGURES = (1, 2, 3), (1, 3), (1, 5), (1, 3)
TICKS = (24, 6, 48)
RANGES = ((55, 84), (60, 72), (55, 90))
MARKS = (None, 5, 2)
GAPS = (8, 7, 0)
VALUE_KINDS = ('random', 'flat', 'nan and inf', 'clamped')


def panel_values(kind, f, k, seed):
    """-> (values (f, k) fp32, vmin, vmax as given to the call)"""
    rs = np.random.RandomState(seed)
    v = rs.rand(f, k).astype(np.float32)
    if kind == 'flat':
        return np.full((f, k), 0.25, np.float32), None, None
    if kind == 'nan and inf':
        v = (v - np.float32(0.5)) * np.float32(3.0)
        v.flat[0] = np.nan
        if v.size > 1:
            v.flat[1], v.flat[-1] = np.inf, -np.inf
        else:
            v.flat[0] = np.inf if seed % 2 else np.nan
        return v, None, None
    if kind == 'clamped':
        return v * np.float32(4.0) - np.float32(1.0), 0.0, 1.0
    return v, None, None


def raster_cases():
    """[dict]: the full product of pixel sizes, measures, figures and with / without values; ticks, pitch range, mark, gap and the
    kind of values cycle through it"""
    out = []
    for i, (ppt, ppp, k, f, with_values) in enumerate(itertools.product(PX_PER_TWELFTH, PX_PER_PITCH, MEASURES, FIGURES, (False, True))):
        lo, hi = RANGES[(i // 2) % 3]
        case = dict(px_per_twelfth=ppt, px_per_pitch=ppp, k=k, f=f, t=TICKS[(i // 4) % 3], pitch_lo=lo, pitch_hi=hi,
                    mark=MARKS[(i // 2 + i // 6) % 3], gap=GAPS[(i // 2) % 3], with_values=with_values, kind=VALUE_KINDS[(i // 2) % 4],
                    seed=i)
        out.append(case)
    return out


def case_inputs(case):
    """-> (score (f, k, t), values or None, vmin, vmax, the look's keywords)"""
    f, k, t = case['f'], case['k'], case['t']
    score = measures(f * k, t, case['seed']).reshape(f, k, t)
    values, vmin, vmax = panel_values(case['kind'], f, k, case['seed']) if case['with_values'] else (None, None, None)
    look = {key: case[key] for key in ('pitch_lo', 'pitch_hi', 'px_per_twelfth', 'px_per_pitch', 'mark', 'gap')}
    return score, values, vmin, vmax, look


def situations(case):
    """what a case reaches, as a set of names"""
    _, _, midi, is_note, slur, _ = vocabulary()
    score, values, vmin, vmax, look = case_inputs(case)
    f, k, t = score.shape
    ev = events(score.reshape(f * k, t), midi, is_note, slur)
    mark = default_mark(look['px_per_twelfth']) if look['mark'] is None else look['mark']
    lo, hi = look['pitch_lo'], look['pitch_hi']
    seen = {f'px_per_twelfth {look["px_per_twelfth"]}', f'px_per_pitch {look["px_per_pitch"]}', f'K {k}', f'F {f}',
            'values' if values is not None else 'no values'}
    _, _, w = geometry(k, t, values is not None, lo, hi, look['px_per_twelfth'], look['px_per_pitch'], 12, look['gap'])
    if (3 * w) % 4:
        seen.add('odd row')
    for onset, length, pitch in sounding(ev):
        seen.add('below' if pitch < lo - 1 else 'above' if pitch > hi + 1 else 'low edge' if pitch == lo else 'high edge' if pitch == hi
                 else 'mark row only' if pitch in (lo - 1, hi + 1) else 'inside')
        if (onset + length) % (2 * t) == 0 and length * look['px_per_twelfth'] < mark:
            seen.add('mark cut by a measure end')
    if values is not None:
        vlo, vhi = value_bounds(values, vmin, vmax)
        seen |= {name for name, on in (('vmin == vmax', vlo == vhi), ('nan', np.isnan(values).any()), ('inf', np.isinf(values).any()),
                                       ('clamped', (values[np.isfinite(values)] > vhi).any())) if on}
    return seen


REACHED = {'px_per_twelfth 1', 'px_per_twelfth 2', 'px_per_twelfth 3', 'px_per_pitch 1', 'px_per_pitch 3', 'K 1', 'K 5', 'F 1', 'F 3',
           'values', 'no values', 'odd row', 'below', 'above', 'low edge', 'high edge', 'mark row only', 'inside',
           'mark cut by a measure end', 'vmin == vmax', 'nan', 'inf', 'clamped'}

"""MIDI files and piano rolls without a GPU: the ABI of the new entry points and their host checks, the integer restatement of the
note events against a fractions.Fraction transcription of the reference's conversion, the MIDI writer and reader, the way back from
notes to tokens, the case table of the raster test, and the surface of the trainer and the command line."""
import ctypes
import inspect
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import arvae_amd  # noqa: E402,F401
import pianoroll_cases as pc  # noqa: E402
from arvae_amd import midi  # noqa: E402

NAMES = ('arvae_measure_notes', 'arvae_render_pianoroll_bytes', 'arvae_render_pianoroll')


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
    assert any(os.path.basename(s) == 'pianoroll.hip' for s in build.sources())


def test_bytes_equal_the_restatement(lib):
    for case in pc.raster_cases():
        _, _, _, _, look = pc.case_inputs(case)
        h, _, w = pc.geometry(case['k'], case['t'], case['with_values'], look['pitch_lo'], look['pitch_hi'], look['px_per_twelfth'],
                              look['px_per_pitch'], 12, look['gap'])
        assert lib.arvae_render_pianoroll_bytes(case['k'], case['t'], look['pitch_lo'], look['pitch_hi'], look['px_per_twelfth'],
                                                look['px_per_pitch'], int(case['with_values']), 12, look['gap']) == h * w * 3
    assert lib.arvae_render_pianoroll_bytes(5, 24, 55, 84, 2, 4, 1, 12, 8) == 120 * (480 + 8 + 60) * 3      # the default figure


def test_host_checks_refuse_before_any_launch(lib):
    """pure host code: every call returns ARVAE_E_INVALID with a message before a launch (the pointers are never dereferenced)"""
    p = ctypes.c_void_p(64)

    def render(score=p, f=2, k=5, t=24, midi_lut=p, is_note=p, v=35, slur=0, values=p, vmin=0.0, vmax=1.0, lo=55, hi=84, ppt=2, ppp=4,
               mark=1, cell=12, gap=8, radius=3, out=p):
        return lib.arvae_render_pianoroll(score, f, k, t, midi_lut, is_note, v, slur, values, vmin, vmax, lo, hi, ppt, ppp, mark, cell, gap,
                                          radius, out, None)

    def notes(score=p, m=4, t=24, midi_lut=p, is_note=p, v=35, slur=0, out=p):
        return lib.arvae_measure_notes(score, m, t, midi_lut, is_note, v, slur, out, None)

    def message():
        return lib.arvae_last_error_string()

    for null in ('score', 'midi_lut', 'is_note', 'out'):
        assert render(**{null: None}) == -1 and b'null' in message()
        assert notes(**{null: None}) == -1 and b'null' in message()
    for t in (0, 5, 25, -6):
        assert render(t=t) == -1 and b'multiple of 6' in message()
        assert notes(t=t) == -1 and b'multiple of 6' in message()
        assert lib.arvae_render_pianoroll_bytes(5, t, 55, 84, 2, 4, 0, 12, 8) == -1
    assert render(lo=85, hi=84) == -1 and b'pitch' in message()
    assert render(lo=-1) == -1 and render(hi=128) == -1
    for zero in ('ppt', 'ppp'):
        assert render(**{zero: 0}) == -1 and b'positive' in message()
    assert render(cell=0) == -1 and render(gap=-1) == -1 and render(radius=-1) == -1 and render(mark=-1) == -1
    assert render(f=0) == -1 and render(k=0) == -1 and notes(m=0) == -1
    assert render(slur=35) == -1 and notes(slur=-1) == -1 and b'slur' in message()
    assert render(vmin=1.0, vmax=0.0) == -1 and render(vmin=float('nan')) == -1 and render(vmax=float('inf')) == -1
    # 2^31 bytes and more: one beat of 30 pitches has 1080 bytes per pixel of a twelfth, and 2^31 / 1080 = 1988410.07
    assert lib.arvae_render_pianoroll_bytes(1, 6, 55, 84, 1988411, 1, 0, 12, 8) == -1 and b'2^31' in message()
    assert lib.arvae_render_pianoroll_bytes(1, 6, 55, 84, 1988410, 1, 0, 12, 8) == 30 * 12 * 1988410 * 3
    assert render(ppt=1988411, ppp=1, k=1, t=6, values=None) == -1 and b'2^31' in message()
    assert render(ppt=2 ** 31 - 1, ppp=2 ** 31 - 1, k=2 ** 31 - 1, t=2 ** 31 - 2, cell=2 ** 31 - 1, gap=2 ** 31 - 1) == -1 and b'2^31' in message()


def test_wrappers_refuse():
    import torch
    from arvae_amd import ops
    _, _, midi_lut, is_note, slur, _ = pc.vocabulary()
    tables = (torch.from_numpy(midi_lut), torch.from_numpy(is_note))
    score = torch.zeros(2, 5, 24, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.measure_notes(score[0], tables, slur=slur)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.render_pianoroll(score, tables, slur=slur)
    with pytest.raises(ValueError, match='multiple of 6'):
        ops.measure_notes(score[0, :, :23], tables, slur=slur)
    with pytest.raises(TypeError):
        ops.measure_notes(score[0].int(), tables, slur=slur)
    with pytest.raises(ValueError):
        ops.render_pianoroll(score[0], tables, slur=slur)
    with pytest.raises(TypeError, match='slur'):         # no default: the slur's index differs from vocabulary to vocabulary
        ops.measure_notes(score[0], tables)
    with pytest.raises(TypeError, match='slur'):
        ops.render_pianoroll(score, tables)
    assert ops.pianoroll_geometry(5, 24) == (120, 480) and ops.pianoroll_geometry(5, 24, True) == (120, 548)
    assert ops.pianoroll_geometry(1, 6, True, 55, 90, 3, 1, 10, 7) == (36, 36 + 7 + 10)


# ---- the events: the integer restatement against the reference's conversion in fractions ------------------------------------------------
def _timeline(elements, twelfths):
    """[(offset, quarter length, pitch)] -> the pitch sounding in every twelfth, and the onsets of the sounding notes"""
    line = np.zeros(twelfths, np.int64)
    for at, dur, pitch in elements:
        a, b = at * 12, (at + dur) * 12
        assert a.denominator == 1 and b.denominator == 1
        line[int(a):int(b)] = pitch
    return line


def test_events_agree_with_the_fraction_transcription():
    i2n, _, midi_lut, is_note, slur, v = pc.vocabulary()
    corners = pc.corner_rows()
    rows = np.concatenate([np.stack([r for name, r in corners.items() if name != 'token -1 and V']), pc.random_measures(300, 24, seed=1),
                           pc.random_measures(100, 24, seed=2, p_slur=0.9), pc.random_measures(50, 24, seed=3, p_slur=0.0)])
    ev = pc.events(rows, midi_lut, is_note, slur)
    for r, row in enumerate(rows):                       # every measure by itself
        ref = pc.m21_sequence([row], i2n, slur)
        assert sum(d for _, d, _ in ref) == 4
        want = sorted((int(a * 12), int(d * 12), p) for a, d, p in ref if p > 0)
        assert sorted(pc.sounding(ev[r:r + 1])) == want, (r, row)
        line = _timeline(ref, 48)
        got = np.repeat(ev[r, :, 0], [pc.tick_twelfth(t + 1) - pc.tick_twelfth(t) for t in range(24)])
        assert np.array_equal(got, line), (r, row)
        starts = ev[r, :, 1]                               # the element of a tick is the last non-slur tick up to it
        for t in range(24):
            before = [s for s in range(t + 1) if row[s] != slur]
            assert starts[t] == (before[-1] if before else -1)
        assert all((ev[r, t, 2] > 0) == (row[t] != slur) for t in range(24))
    seq = pc.m21_sequence(rows[:40], i2n, slur)          # and a sequence of them: measure k starts at 4 k
    assert sorted(pc.sounding(ev[:40])) == sorted((int(a * 12), int(d * 12), p) for a, d, p in seq if p > 0)
    assert np.array_equal(_timeline(seq, 40 * 48), np.concatenate([np.repeat(ev[r, :, 0], [3, 1, 2, 2, 1, 3] * 4) for r in range(40)]))
    # the tick grid itself
    assert [Fraction(pc.tick_twelfth(t), 12) for t in range(6)] == pc.TICK_VALUES
    assert [Fraction(pc.tick_twelfth(t + 1) - pc.tick_twelfth(t), 12) for t in range(24)] == pc.TICK_DURATIONS * 4
    assert [midi.tick_twelfth(t) for t in range(49)] == [pc.tick_twelfth(t) for t in range(49)] and pc.tick_twelfth(24) == 48
    # tokens outside the vocabulary are silence and begin an element
    row = corners['token -1 and V'][None]
    e = pc.events(row, midi_lut, is_note, slur)[0]
    assert e[:6].tolist() == [[67, 0, 4], [67, 0, 0], [0, 2, 4], [0, 2, 0], [0, 4, 40], [0, 4, 0]]
    assert pc.events(corners['all slurs'][None], midi_lut, is_note, slur)[0].tolist() == [[0, -1, 0]] * 24


# ---- MIDI files -----------------------------------------------------------------------------------------------------------------------
def test_midi_round_trip_of_events(tmp_path):
    _, _, midi_lut, is_note, slur, _ = pc.vocabulary()
    rows = np.concatenate([np.stack(list(pc.corner_rows().values())), pc.random_measures(20, 24, seed=4)])
    ev = pc.events(rows, midi_lut, is_note, slur)
    path = midi.write_midi(str(tmp_path / 'a.mid'), ev)
    division, notes = midi.read_midi(path)
    assert division == 480 and notes == [(on * 40, d * 40, p) for on, d, p in sorted(pc.sounding(ev))]
    assert midi.notes_from_events(ev) == pc.sounding(ev)
    data = open(path, 'rb').read()
    assert data[:14] == b'MThd\x00\x00\x00\x06\x00\x01\x00\x01\x01\xe0' and data[14:18] == b'MTrk'
    assert int.from_bytes(data[18:22], 'big') == len(data) - 22 and data.endswith(b'\xff\x2f\x00')
    assert b'\xff\x51\x03\x07\xa1\x20' in data and b'\xff\x58\x04\x04\x02\x18\x08' in data      # 120 bpm, 4/4
    assert data.count(b'\x90') >= len(notes) and bytes([0x90, notes[0][2], 90]) in data


def test_midi_delta_times_and_ends(tmp_path):
    # delta times at the edges of the variable-length quantity: 127 | 128, 16383 | 16384 (one, two, three bytes)
    notes = [(0, 127, 60), (127, 128, 62), (255, 16383, 64), (255 + 16383, 16384, 65), (255 + 16383 + 16384, 2097152, 67)]
    path = midi.write_midi(str(tmp_path / 'vlq.mid'), notes, unit='tick')
    assert midi.read_midi(path) == (480, notes)
    data = open(path, 'rb').read()
    for vlq in (b'\x7f', b'\x81\x00', b'\xff\x7f', b'\x81\x80\x00', b'\x81\x80\x80\x00'):
        assert vlq + b'\x80' in data, vlq               # each delta stands before a note-off
    # ten silent measures before a note that ends exactly with the last measure: a delta of 10 * 1920 + 1800 ticks
    _, n2i, midi_lut, is_note, slur, _ = pc.vocabulary()
    rows = np.full((11, 24), slur, np.int64)
    rows[10, 23] = n2i['C5']
    ev = pc.events(rows, midi_lut, is_note, slur)
    path = midi.write_midi(str(tmp_path / 'late.mid'), ev)
    assert midi.read_midi(path) == (480, [((10 * 48 + 45) * 40, 3 * 40, 72)])
    assert open(path, 'rb').read().endswith(b'\x80\x48\x00\x00\xff\x2f\x00')      # the track ends with the note, at the barline
    # an empty sequence, and measures without a note: valid files without notes; the second is as long as its measures
    for name, what in (('none.mid', []), ('silent.mid', ev[:3]), ('zero.mid', np.zeros((0, 24, 3), np.int32))):
        path = midi.write_midi(str(tmp_path / name), what)
        assert midi.read_midi(path) == (480, [])
    assert open(str(tmp_path / 'silent.mid'), 'rb').read().endswith(midi._vlq(3 * 1920) + b'\xff\x2f\x00')
    for bad in ([(0, 0, 60)], [(-1, 4, 60)], [(0, 4, 128)]):
        with pytest.raises(ValueError):
            midi.write_midi(str(tmp_path / 'bad.mid'), bad)


def test_read_midi_running_status_and_foreign_events(tmp_path):
    """a hand-made file: running status (note-on with velocity 0 as note-off), a program change, a pitch bend, a text meta event, a
    system-exclusive event and system-common events (song position, song select, tune request, time code) between the notes, a second
    track that ends later"""
    track1 = (b'\x00\xff\x03\x02hi' b'\x00\xc0\x05' b'\x00\x90\x3c\x50' b'\x60\x3c\x00' b'\x00\x3e\x50' b'\x00\xe0\x00\x40'
              b'\x81\x00\x90\x3e\x00' b'\x00\xf0\x02\x01\xf7' b'\x00\xf2\x10\x20' b'\x00\xf3\x05' b'\x00\xf6' b'\x00\xf1\x33'
              b'\x00\x90\x40\x40' b'\x0a\x80\x40\x00' b'\x00\xff\x2f\x00')
    track2 = b'\x05\x91\x30\x40' b'\x05\x30\x00' b'\x83\x00\xff\x2f\x00'
    data = b'MThd' + (6).to_bytes(4, 'big') + b'\x00\x01\x00\x02\x00\x60'
    for tr in (track1, track2):
        data += b'MTrk' + len(tr).to_bytes(4, 'big') + tr
    path = tmp_path / 'hand.mid'
    path.write_bytes(data)
    assert midi.read_midi(str(path)) == (96, [(0, 96, 60), (5, 5, 48), (96, 128, 62), (224, 10, 64)])
    assert midi.read_midi(str(path), with_length=True)[2] == 10 + 384       # the later of the two end-of-track events
    (tmp_path / 'not.mid').write_bytes(b'RIFF' + bytes(20))
    with pytest.raises(ValueError):
        midi.read_midi(str(tmp_path / 'not.mid'))


def canonical(rows, i2n, n2i):
    """tokens with the same events in canonical form: the symbol at an element's first tick, 'rest' where silence begins"""
    out = np.full_like(rows, n2i['__'])
    for r, row in enumerate(rows):
        silent = None
        for t, x in enumerate(row):
            if x == n2i['__'] and t > 0:
                continue
            now_silent = x == n2i['__'] or i2n[int(x)] in ('rest', 'START', 'END', None)
            if now_silent and silent:
                continue                                 # silence goes on
            out[r, t] = n2i['rest'] if now_silent else x
            silent = now_silent
    return out


def test_tokens_from_notes_inverts_the_events(tmp_path):
    i2n, n2i, midi_lut, is_note, slur, _ = pc.vocabulary()
    rows = np.concatenate([np.stack([r for name, r in pc.corner_rows().items() if name != 'token -1 and V']), pc.random_measures(200, 24, seed=6)])
    want = canonical(rows, i2n, n2i)
    ev = pc.events(rows, midi_lut, is_note, slur)
    assert np.array_equal(pc.events(want, midi_lut, is_note, slur)[:, :, 0], ev[:, :, 0])          # the canonical form sounds the same
    got = np.array(midi.tokens_from_notes(pc.sounding(ev), n2i, len(rows)))
    assert got.shape == rows.shape
    assert np.array_equal(got, want)                     # (a note struck again at the same pitch is a note of its own)
    path = midi.write_midi(str(tmp_path / 'a.mid'), ev)
    division, notes = midi.read_midi(path)
    assert np.array_equal(np.array(midi.tokens_from_notes(notes, n2i, len(rows), division=division)), want)
    assert np.array_equal(canonical(want, i2n, n2i), want)
    # a note across a barline begins again in the next measure
    two = midi.tokens_from_notes([(45, 3 + 48 + 3, 67)], n2i, 3)
    assert two[0][23] == two[1][0] == two[2][0] == n2i['G4'] and two[2][1] == n2i['rest'] and two[0][0] == n2i['rest']


def test_measures_of_a_file_include_its_silent_end(tmp_path):
    """the command line's reader counts the measures by the track's length: silence after the last note stays"""
    import train_measure_vae
    _, n2i, midi_lut, is_note, slur, _ = pc.vocabulary()
    rows = np.full((4, 24), slur, np.int64)
    rows[1, 6] = n2i['C5']
    path = midi.write_midi(str(tmp_path / 'quiet.mid'), pc.events(rows, midi_lut, is_note, slur))
    assert midi.read_midi(path, with_length=True) == (480, [((48 + 12) * 40, 36 * 40, 72)], 4 * 1920)
    got = train_measure_vae.measures_of_midi(path, n2i)
    assert got.shape == (4, 24) and got[1].tolist() == [n2i['rest']] + [slur] * 5 + [n2i['C5']] + [slur] * 17
    assert all(got[m].tolist() == [n2i['rest']] + [slur] * 23 for m in (0, 2, 3))
    path = midi.write_midi(str(tmp_path / 'none.mid'), [])
    assert train_measure_vae.measures_of_midi(path, n2i).shape == (1, 24)


def test_tokens_from_notes_refuses():
    _, n2i, _, _, _, _ = pc.vocabulary()
    for bad, word in (([(1, 3, 67)], 'grid'), ([(0, 2, 67)], 'grid'), ([(0, 6, 67), (4, 4, 69)], 'overlap'), ([(0, 3, 30)], 'vocabulary'),
                      ([(0, 3, 100)], 'vocabulary'), ([(45, 6, 67)], 'after measure'), ([(0, 0, 67)], 'duration')):
        with pytest.raises(ValueError, match=word):
            midi.tokens_from_notes(bad, n2i, 1)
    with pytest.raises(ValueError, match='grid'):
        midi.tokens_from_notes([(0, 130, 67)], n2i, 1, division=480)       # 130 MIDI ticks are no whole twelfth
    assert midi.tokens_from_notes([(0, 120, 67)], n2i, 1, division=480)[0][:2] == [n2i['G4'], n2i['rest']]


# ---- the raster's oracle and its case table -----------------------------------------------------------------------------------------------
def test_case_table_reaches_what_it_is_there_for():
    cases = pc.raster_cases()
    assert len(cases) == 48
    seen = set()
    for case in cases:
        seen |= pc.situations(case)
    assert pc.REACHED <= seen, pc.REACHED - seen


def test_restatement_of_the_raster_by_hand():
    """one measure, one note: every layer where the issue puts it"""
    _, n2i, midi_lut, is_note, slur, _ = pc.vocabulary()
    row = np.full((1, 1, 6), slur, np.int64)
    row[0, 0, 1] = n2i['A3']                             # MIDI 57 from twelfth 3 to the end (9 twelfths)
    img = pc.pianoroll(row, midi_lut, is_note, slur, np.array([[0.5]], np.float32), 0.0, 1.0, pitch_lo=55, pitch_hi=58, px_per_twelfth=2,
                       px_per_pitch=2, mark=3, panel_cell=6, gap=2, dot_radius=1)
    assert img.shape == (1, 8, 24 + 2 + 6, 3)
    shade = {tuple(255 - (v * (255 - pc.DARK) + 63) // 127): v for v in (0, 30, 50, 90, 100, 127)}
    v = np.array([[shade[tuple(px)] for px in line[:24]] for line in img[0]])
    assert v[:, 0].tolist() == [100] * 8                 # the measure line
    assert v[0].tolist()[1:6] == [30] * 5 and v[2].tolist()[1:6] == [0] * 5          # 58 is even, 57 odd
    assert v[2].tolist()[6:] == [127] * 3 + [90] * 15 and v[3].tolist() == v[2].tolist()          # the note's rows: mark, then the note
    assert v[0].tolist()[6:] == [127] * 3 + [30] * 15 and v[4].tolist()[6:] == [127] * 3 + [30] * 15          # the mark's rows above and below
    assert v[6].tolist() == [100] + [0] * 23
    assert (img[0, :, 24:26] == 255).all()               # the gap
    assert shade[(8, 48, 107)] == 127 and shade[(255, 255, 255)] == 0
    row_of_disc = 8 - 1 - int(np.floor(np.float32(0.5) * np.float32(7) + np.float32(0.5)))
    assert row_of_disc == 3 and pc.disc_row(0.5, 0.0, 1.0, 8) == 3
    panel = img[0, :, 26:, 0]
    assert (panel == 0).sum() == 5 and panel[3, 3] == 0 and panel[2, 3] == 0 and panel[3, 2] == 0 and panel[2, 2] == 255
    assert pc.default_mark(1) == pc.default_mark(2) == 1 and pc.default_mark(4) == 2 and pc.default_mark(10) == 6


# ---- trainer and command line ---------------------------------------------------------------------------------------------------------------
def test_trainer_and_cli_surface(capsys):
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer, pitch_to_midi
    sig = inspect.signature(MeasureVAETrainer.plot_latent_interpolations).parameters
    assert [(k, v.default) for k, v in sig.items()][1:6] == [('latent_codes', inspect._empty), ('attr_str', inspect._empty), ('num_points', 10),
                                                             ('dim', None), ('sweep_points', 5)]
    sig = inspect.signature(MeasureVAETrainer.write_measures).parameters
    assert [(k, v.default) for k, v in sig.items()][1:5] == [('tensor_score', inspect._empty), ('stem', inspect._empty), ('values', None),
                                                             ('attr_str', None)]
    assert pitch_to_midi is midi.pitch_to_midi and pitch_to_midi('G3') == 55 and pitch_to_midi('B-4') == 70
    import train_measure_vae
    with pytest.raises(SystemExit) as e:
        train_measure_vae.run(['--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--plots' in out and '--write_midi' in out and '--from_midi' in out
    for args in (['--write_midi', 'x'], ['--from_midi', 'x.mid'], ['--infill', '1', '--keep_ticks', '0-5', '--from_midi', '/nonexistent.mid']):
        with pytest.raises(ValueError):
            train_measure_vae.run(args)

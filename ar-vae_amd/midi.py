"""Standard MIDI Files of decoded measures, in plain Python: what the reference gets from music21's score.write('midi').

Times are counted in twelfths of a quarter note, the unit of ops.measure_notes: tick t of a 24-tick measure starts at twelfth
12 (t // 6) + TICK_START[t % 6] and lasts TICK_LENGTH[t % 6] (TICK_VALUES / compute_tick_durations of the reference's
bar_dataset_helpers.py, times 12); a measure has 48 twelfths.  A note is (onset, duration, pitch).
"""
import struct

TICK_START = (0, 3, 4, 6, 8, 9)
TICK_LENGTH = (3, 1, 2, 2, 1, 3)
DIVISION = 480                      # MIDI ticks per quarter note: 40 per twelfth
_PITCH = {'C': 0, 'D': 2, 'E': 4, 'F': 5, 'G': 7, 'A': 9, 'B': 11}
NON_NOTES = ('__', 'START', 'END', 'rest', None)        # vocabulary entries without a pitch (build_measure_tables reads it too)


def pitch_to_midi(name):
    """'G3', 'F#4', 'B-4' / 'Bb4' -> MIDI number (what music21.pitch.Pitch(name).midi gives)."""
    step, rest = name[0].upper(), name[1:]
    acc = 0
    while rest and rest[0] in '#-b':
        acc += 1 if rest[0] == '#' else -1
        rest = rest[1:]
    return 12 * (int(rest) + 1) + _PITCH[step] + acc


def tick_twelfth(t):
    """the twelfth at which tick t of a measure starts (t = T: the measure's length)"""
    return 12 * (t // 6) + TICK_START[t % 6]


def notes_from_events(events):
    """(M, T, 3) note events of a sequence of measures (ops.measure_notes, copied to the host) -> [(onset, duration, pitch)] in
    twelfths from the start of the first measure; silent elements are left out"""
    rows = events.tolist() if hasattr(events, 'tolist') else list(events)
    notes = []
    for m, row in enumerate(rows):
        for t, (pitch, _, length) in enumerate(row):
            if length > 0 and pitch > 0:
                notes.append((m * 2 * len(row) + tick_twelfth(t), int(length), int(pitch)))
    return notes


def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    return bytes(reversed(out))


def write_midi(path, notes_or_events, unit='twelfth', length=None, tempo=120, velocity=90):
    """A format-1 file with one track at division 480: tempo and 4/4 meta events, then note-on (velocity 90) / note-off on channel 0
    with variable-length delta times, then end-of-track.  notes_or_events: the (M, T, 3) events of a sequence of measures, or a
    list of (onset, duration, pitch); unit 'twelfth' (40 MIDI ticks) or 'tick'.  length: where the track ends, in `unit` (events: the
    end of the last measure; never before the last note's end).  An empty sequence gives a valid file without notes."""
    if unit not in ('twelfth', 'tick'):
        raise ValueError(f"unit is 'twelfth' or 'tick', got {unit!r}")
    if hasattr(notes_or_events, 'ndim') or hasattr(notes_or_events, 'dim'):
        shape = tuple(notes_or_events.shape)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f'note events are (M, T, 3), got {shape}')
        unit = 'twelfth'                                 # (what events are counted in)
        if length is None:
            length = shape[0] * 2 * shape[1]
        notes = notes_from_events(notes_or_events)
    else:
        notes = [(int(on), int(dur), int(p)) for on, dur, p in notes_or_events]
    scale = DIVISION // 12 if unit == 'twelfth' else 1
    changes = []                                         # (time, 0 = off / 1 = on, pitch): at equal times a note ends before the next begins
    for on, dur, pitch in notes:
        if on < 0 or dur <= 0 or not 0 <= pitch <= 127:
            raise ValueError(f'a note is (onset >= 0, duration > 0, pitch in [0, 127]), got {(on, dur, pitch)}')
        changes += [(on * scale, 1, pitch), ((on + dur) * scale, 0, pitch)]
    changes.sort(key=lambda c: (c[0], c[1]))
    track = bytearray()
    track += _vlq(0) + b'\xff\x51\x03' + struct.pack('>I', round(60_000_000 / tempo))[1:]
    track += _vlq(0) + b'\xff\x58\x04\x04\x02\x18\x08'
    now = 0
    for time, on, pitch in changes:
        track += _vlq(time - now) + bytes([0x90 if on else 0x80, pitch, velocity if on else 0])
        now = time
    end = max(now, 0 if length is None else int(length) * scale)
    track += _vlq(end - now) + b'\xff\x2f\x00'
    with open(path, 'wb') as f:
        f.write(b'MThd' + struct.pack('>IHHH', 6, 1, 1, DIVISION) + b'MTrk' + struct.pack('>I', len(track)) + bytes(track))
    return path


_SYSTEM_DATA_BYTES = {0xF1: 1, 0xF2: 2, 0xF3: 1}         # MIDI time code, song position, song select; the other 0xF4-0xFE take none


def read_midi(path, with_length=False):
    """-> (division, [(onset, duration, pitch)]) in MIDI ticks, sorted by onset, of every note of every track; meta, system
    exclusive, system common and realtime events are skipped by their lengths, running status and note-on at velocity 0 (a
    note-off) are understood.  with_length=True: -> (division, notes, length), length the tick of the latest end-of-track, which
    lies after the last note's end where the file closes with silence."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:4] != b'MThd' or len(data) < 14:
        raise ValueError(f'{path}: not a Standard MIDI File')
    header_len, _, n_tracks, division = struct.unpack('>IHHH', data[4:14])
    if division & 0x8000:
        raise ValueError(f'{path}: SMPTE time division is not supported')
    pos, notes, length = 8 + header_len, [], 0
    for _ in range(n_tracks):
        if data[pos:pos + 4] != b'MTrk':
            raise ValueError(f'{path}: track chunk expected at byte {pos}')
        end = pos + 8 + struct.unpack('>I', data[pos + 4:pos + 8])[0]
        pos += 8
        now, status, sounding = 0, None, {}
        while pos < end:
            delta = 0
            while True:
                byte = data[pos]
                pos += 1
                delta = (delta << 7) | (byte & 0x7F)
                if not byte & 0x80:
                    break
            now += delta
            if data[pos] & 0x80:
                status = data[pos]
                pos += 1
            elif status is None:
                raise ValueError(f'{path}: data byte without a status at byte {pos}')
            if status == 0xFF or status in (0xF0, 0xF7):
                if status == 0xFF:
                    pos += 1                             # the meta type
                size = 0
                while True:
                    byte = data[pos]
                    pos += 1
                    size = (size << 7) | (byte & 0x7F)
                    if not byte & 0x80:
                        break
                pos += size
                status = None                            # (meta and sysex events cancel running status)
                continue
            if status >= 0xF1:
                pos += _SYSTEM_DATA_BYTES.get(status, 0)
                status = None                            # (system common cancels running status; realtime bytes do not occur in files)
                continue
            kind = status & 0xF0
            key = (status & 0x0F, data[pos])
            if kind == 0x90 and data[pos + 1] > 0:
                sounding.setdefault(key, []).append(now)
            elif kind in (0x80, 0x90) and sounding.get(key):
                start = sounding[key].pop(0)
                notes.append((start, now - start, key[1]))
            pos += 1 if kind in (0xC0, 0xD0) else 2
        pos, length = end, max(length, now)
    return (division, sorted(notes), length) if with_length else (division, sorted(notes))


def tokens_from_notes(notes, note2index, num_measures, division=None, ticks=24):
    """Grid-aligned monophonic notes -> canonical tokens, num_measures rows of `ticks`: an element's symbol at its first tick, 'rest'
    where silence begins (the start of a measure included), '__' elsewhere; a note that crosses a barline begins again in the next
    measure, as nothing ties across one.  notes: (onset, duration, pitch) in twelfths, or in MIDI ticks with `division` (read_midi's).
    Nothing is quantised: ValueError for an onset or end that is no tick of the grid, for overlapping notes, for a note past the last
    measure and for a pitch the vocabulary lacks."""
    if division is not None:
        if division % 12:
            raise ValueError(f'division {division} has no whole twelfths')
        per = division // 12
        for on, dur, _ in notes:
            if on % per or dur % per:
                raise ValueError(f'note at MIDI tick {on} lasting {dur} is off the grid (a twelfth is {per} ticks)')
        notes = [(on // per, dur // per, p) for on, dur, p in notes]
    by_pitch = {}
    for sym, idx in sorted(note2index.items(), key=lambda kv: kv[1]):
        if sym not in NON_NOTES:
            by_pitch.setdefault(pitch_to_midi(sym), idx)
    slur, rest = note2index['__'], note2index['rest']
    per_measure = 2 * ticks

    def tick_of(w, what):
        m, r = divmod(w, per_measure)
        beat, sub = divmod(r, 12)
        if sub not in TICK_START:
            raise ValueError(f'{what} at twelfth {w} is off the {ticks}-tick grid')
        return m * ticks + beat * 6 + TICK_START.index(sub)

    flat = [slur] * (num_measures * ticks)
    for m in range(num_measures):
        flat[m * ticks] = rest
    last_end = 0
    for on, dur, pitch in sorted(notes):
        if dur <= 0:
            raise ValueError(f'note at twelfth {on} has no duration')
        if on < last_end:
            raise ValueError(f'the note at twelfth {on} overlaps the one before it (monophonic measures only)')
        if pitch not in by_pitch:
            raise ValueError(f'MIDI pitch {pitch} is not in the vocabulary')
        first, end = tick_of(on, 'an onset'), tick_of(on + dur, 'a note end')
        if end > num_measures * ticks:
            raise ValueError(f'the note at twelfth {on} ends after measure {num_measures}')
        flat[first] = by_pitch[pitch]
        for bar in range(first // ticks + 1, (end + ticks - 1) // ticks):
            flat[bar * ticks] = by_pitch[pitch]          # the note goes on across a barline: struck again
        if end < num_measures * ticks and flat[end] == slur:
            flat[end] = rest                             # silence begins (a later note may replace it)
        last_end = on + dur
    return [flat[m * ticks:(m + 1) * ticks] for m in range(num_measures)]

"""MIDI files and piano rolls on the GPU: arvae_measure_notes and arvae_render_pianoroll against the restatements of
tests/pianoroll_cases.py (exact integers, exact bytes), their output bounds and stream, MeasureVAETrainer.write_measures and
plot_latent_interpolations read back from the files they write, and the command line's --write_midi, --plots and --from_midi."""
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
import pianoroll_cases as pc  # noqa: E402
from arvae_amd import midi  # noqa: E402
from test_data_gpu import write_folk  # noqa: E402
from test_sampling import _FolkDataset  # noqa: E402

pytestmark = pytest.mark.gpu
I2N, N2I, MIDI_LUT, IS_NOTE, SLUR, V = pc.vocabulary()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def tables(dev):
    return torch.from_numpy(MIDI_LUT).to(dev), torch.from_numpy(IS_NOTE).to(dev)


def render(dev, score, values=None, vmin=None, vmax=None, **look):
    from arvae_amd import ops
    v = None if values is None else torch.from_numpy(values).to(dev)
    return ops.render_pianoroll(torch.from_numpy(score).to(dev), tables(dev), v, vmin, vmax, slur=SLUR, **look)


# ---- 1. events ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [6, 24, 48])
@pytest.mark.parametrize('m', [1, 63, 257])
def test_measure_notes_equal_the_restatement(dev, m, t):
    """every corner row of pianoroll_cases.corner_rows (one row: the tokens -1 and V) plus random rows; 16 guard words either side"""
    from arvae_amd import ops
    rows = pc.measures(m, t, seed=10 * m + t) if m > 1 else pc.corner_rows(t)['token -1 and V'][None]
    assert rows.shape == (m, t) and (m == 1 or m >= len(pc.corner_rows(t)))
    want = pc.events(rows, MIDI_LUT, IS_NOTE, SLUR)
    buf = torch.full((16 + m * t * 3 + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    out = buf[16:16 + m * t * 3]
    got = ops.measure_notes(torch.from_numpy(rows).to(dev), tables(dev), slur=SLUR, out=out)
    assert got.shape == (m, t, 3) and got.dtype == torch.int32 and got.data_ptr() == out.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want)
    host = buf.cpu().numpy()
    assert np.all(host[:16] == 0x5A5A5A5A) and np.all(host[-16:] == 0x5A5A5A5A)
    again = ops.measure_notes(torch.from_numpy(rows).to(dev)[:, None], tables(dev), slur=SLUR)          # (M, 1, T), the decoder's shape
    assert np.array_equal(again.cpu().numpy(), want)


# ---- 2. raster ----------------------------------------------------------------------------------------------------------------------
def test_raster_is_exact(dev):
    """all 48 cases byte for byte (tiny figures, one launch each); what they reach is asserted in test_pianoroll.py and here"""
    seen = set()
    for case in pc.raster_cases():
        score, values, vmin, vmax, look = pc.case_inputs(case)
        want = pc.pianoroll(score, MIDI_LUT, IS_NOTE, SLUR, values, vmin, vmax, **look)
        got = render(dev, score, values, vmin, vmax, **look).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == want.shape, case
        assert np.array_equal(got, want), (case, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
        seen |= pc.situations(case)
    assert pc.REACHED <= seen, pc.REACHED - seen


def test_default_look(dev):
    """five measures with their attribute beside them, every keyword at its default: 120 x 548, the reference's folk range"""
    score = pc.measures(10, 24, seed=77).reshape(2, 5, 24)
    values = np.random.RandomState(1).rand(2, 5).astype(np.float32)
    got = render(dev, score, values).cpu().numpy()
    assert got.shape == (2, 120, 480 + 8 + 60, 3)
    assert np.array_equal(got, pc.pianoroll(score, MIDI_LUT, IS_NOTE, SLUR, values))
    assert np.array_equal(render(dev, score).cpu().numpy(), pc.pianoroll(score, MIDI_LUT, IS_NOTE, SLUR))
    bach = render(dev, score, pitch_hi=90).cpu().numpy()
    assert bach.shape == (2, 144, 480, 3) and np.array_equal(bach, pc.pianoroll(score, MIDI_LUT, IS_NOTE, SLUR, pitch_hi=90))


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_output_stays_inside_its_buffer(dev, offset):
    """out inside a larger buffer, 64 guard bytes of 0xA5 either side; with offset 1..3 it starts off a 4-byte boundary.  Three
    figures of 36 x 50 pixels (rows of 150 bytes, a whole number of words in all) and three of 35 x 43 (rows of 129 bytes, 13545
    bytes in all: the last word is partial at every offset)"""
    from arvae_amd import ops
    for pitch_hi, gap in ((90, 7), (89, 0)):
        score = pc.measures(3, 6, seed=5).reshape(3, 1, 6)
        values = np.array([[0.0], [np.nan], [1.0]], np.float32)
        look = dict(pitch_lo=55, pitch_hi=pitch_hi, px_per_twelfth=3, px_per_pitch=1, gap=gap, panel_cell=7)
        want = pc.pianoroll(score, MIDI_LUT, IS_NOTE, SLUR, values, **look)
        total = want.size
        assert want.shape == (3, pitch_hi - 54, 36 + gap + 7, 3) and (3 * want.shape[2]) % 4 != 0 and (total % 4 != 0) == (gap == 0)
        buf = torch.full((64 + 4 + total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 4 == 0
        out = buf[64 + offset:64 + offset + total]
        got = ops.render_pianoroll(torch.from_numpy(score).to(dev), tables(dev), torch.from_numpy(values).to(dev), slur=SLUR, out=out, **look)
        assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 4 == offset and np.array_equal(got.cpu().numpy(), want)
        host = buf.cpu().numpy()
        assert np.all(host[:64 + offset] == 0xA5) and np.all(host[64 + offset + total:] == 0xA5)
        strided = torch.zeros(2 * total, dtype=torch.uint8, device=dev)[::2]             # the right size, not dense: refused before the launch
        with pytest.raises(ValueError, match='contiguous'):
            ops.render_pianoroll(torch.from_numpy(score).to(dev), tables(dev), torch.from_numpy(values).to(dev), slur=SLUR, out=strided, **look)


def test_launches_go_to_the_current_stream(dev):
    """Both launches are captured into a HIP graph on a stream of its own (arvae_amd.graphed.Capture, what the trainers replay steps
    with): a capture records only what is launched on the capturing stream and runs nothing, so outputs that hold the right bytes
    after a replay -- and only after it -- came from launches on the current stream.  Then the same on a plain side stream."""
    from arvae_amd import ops
    from arvae_amd.graphed import Capture
    tb = tables(dev)
    score = torch.from_numpy(pc.measures(100, 24, seed=9).reshape(20, 5, 24)).to(dev)
    values = torch.rand(20, 5, device=dev)
    want = pc.pianoroll(score.cpu().numpy(), MIDI_LUT, IS_NOTE, SLUR, values.cpu().numpy(), 0.0, 1.0)
    want_ev = pc.events(score.cpu().numpy().reshape(100, 24), MIDI_LUT, IS_NOTE, SLUR)
    frames = torch.full(want.shape, 0xA5, dtype=torch.uint8, device=dev)
    events = torch.full((100, 24, 3), -7, dtype=torch.int32, device=dev)

    def both():
        ops.render_pianoroll(score, tb, values, 0.0, 1.0, slur=SLUR, out=frames)       # (bounds given: no host read inside the capture)
        ops.measure_notes(score.view(100, 24), tb, slur=SLUR, out=events)
    cap = Capture(device=dev)
    cap.capture(both)
    torch.cuda.synchronize()
    assert bool((frames == 0xA5).all()) and bool((events == -7).all())       # captured, not run
    cap.replay()
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), want) and np.array_equal(events.cpu().numpy(), want_ev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ops.render_pianoroll(score, tb, values, 0.0, 1.0, slur=SLUR)
        got_ev = ops.measure_notes(score.view(100, 24), tb, slur=SLUR)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_ev.cpu().numpy(), want_ev)


# ---- 3. the trainer -------------------------------------------------------------------------------------------------------------------
def tiny_trainer(tmp_path, monkeypatch):
    """the synthetic vocabulary, hidden size 32: the smallest the one-launch decoder takes"""
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer
    monkeypatch.setenv('ARVAE_MODEL_DIR', str(tmp_path / 'models'))
    torch.manual_seed(0)
    ds = _FolkDataset()
    model = MeasureVAE(ds, 10, 2, 2, 32, 0.5, 16, 2, 32, 0.5, False, 'folk')
    trainer = MeasureVAETrainer(ds, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))
    trainer.cuda()
    model.eval()
    with torch.no_grad():                                # sharper notes: the decoded measures hold more than one symbol
        model.decoder.tick_emb_to_note_emb[0].weight.mul_(4.0)
    return trainer


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == 'RGB', path
        return np.asarray(im).copy()


def midi_notes(tokens):
    """what read_midi returns for a file of these measures"""
    return [(on * 40, d * 40, p) for on, d, p in sorted(pc.sounding(pc.events(tokens, MIDI_LUT, IS_NOTE, SLUR)))]


def check_panel(frame, k, roll_w=None):
    """one disc in each of the k panel cells (12 wide after a gap of 8), none in the roll"""
    roll_w = frame.shape[1] - 8 - 12 * k if roll_w is None else roll_w
    black = (frame == 0).all(axis=2)
    assert not black[:, :roll_w + 8].any()
    for c in range(k):
        cell = black[:, roll_w + 8 + 12 * c:roll_w + 8 + 12 * (c + 1)]
        rows = np.flatnonzero(cell.any(axis=1))
        assert 1 <= cell.sum() <= 29 and rows.max() - rows.min() <= 6 and cell[:, 6].any(), c


def test_plot_latent_interpolations(dev, tmp_path, monkeypatch):
    from arvae_amd import ops
    trainer = tiny_trainer(tmp_path, monkeypatch)
    trainer.metrics = {'interpretability': {'rhy_complexity': (3, 0.5), 'pitch_range': (7, 0.4), 'note_density': (1, 0.3), 'contour': (12, 0.6)}}
    calls, launches, event_launches = [], [], []
    decode, roll, notes_of = trainer.decode_latent_codes, ops.render_pianoroll, ops.measure_notes

    def spy(z, *a, **kw):
        out = decode(z, *a, **kw)
        calls.append((z.detach().cpu().numpy().copy(), out[1].detach().cpu().numpy()[:, 0].copy()))
        return out

    def roll_spy(*a, **kw):
        launches.append(roll(*a, **kw))
        return launches[-1]

    def notes_spy(*a, **kw):
        event_launches.append(notes_of(*a, **kw))
        return event_launches[-1]
    monkeypatch.setattr(trainer, 'decode_latent_codes', spy)
    monkeypatch.setattr(ops, 'measure_notes', notes_spy)
    monkeypatch.setattr(ops, 'render_pianoroll', roll_spy)
    codes = np.random.RandomState(0).randn(7, 16).astype(np.float32)
    paths = trainer.plot_latent_interpolations(codes, 'contour', num_points=3)
    folder = os.path.join(os.path.dirname(trainer.model.filepath), 'results')
    assert paths == [os.path.join(folder, name) for i in range(3)
                     for name in (f'original_{i}.mid', f'latent_interpolations_contour_{i}.mid', f'latent_interpolations_contour_{i}.png')]
    assert sorted(os.listdir(folder)) == sorted(os.path.basename(p) for p in paths)
    assert len(calls) == 1 and len(launches) == 1 and len(event_launches) == 1      # one decoder batch, one render and one events launch
    assert event_launches[0].shape == (3 * 5 + 3, 24, 3)
    z, tokens = calls[0]
    assert z.shape == (3 * 5 + 3, 16) and np.array_equal(z[15:], codes[:3])
    sweep = np.linspace(-4.0, 4.0, 5, dtype=np.float32)
    others = [c for c in range(16) if c != 12]
    for i in range(3):
        assert np.array_equal(z[5 * i:5 * i + 5, 12], sweep) and np.array_equal(z[5 * i:5 * i + 5][:, others], np.repeat(codes[i:i + 1, others], 5, 0))
    shown = tokens[:15].reshape(3, 5, 24).copy()
    shown[:, 2] = tokens[15:]                            # the original in the middle
    labels = trainer.compute_attribute_labels(torch.from_numpy(shown.reshape(15, 24)).to(dev), ['contour']).cpu().numpy().reshape(3, 5)
    want = pc.pianoroll(shown, MIDI_LUT, IS_NOTE, SLUR, labels)
    frames = launches[0].cpu().numpy()
    assert frames.shape == (3, 120, 548, 3) and np.array_equal(frames, want)
    assert len(np.unique(shown)) > 2                     # (the measures are not empty)
    for i in range(3):
        assert midi.read_midi(paths[3 * i]) == (480, midi_notes(tokens[15 + i:16 + i]))
        assert midi.read_midi(paths[3 * i + 1]) == (480, midi_notes(shown[i]))
        png = read_png(paths[3 * i + 2])
        assert np.array_equal(png, frames[i])
        check_panel(png, 5)
    # dim given, another sweep, fewer codes than points
    calls.clear()
    paths = trainer.plot_latent_interpolations(codes[:2], 'note_density', num_points=10, dim=5, sweep_points=3)
    assert len(paths) == 6 and calls[0][0].shape == (2 * 3 + 2, 16) and np.array_equal(calls[0][0][:3, 5], [-4.0, 0.0, 4.0])
    assert read_png(paths[2]).shape == (120, 3 * 96 + 8 + 36, 3)
    with pytest.raises(AssertionError):
        trainer.plot_latent_interpolations(codes, 'contour', sweep_points=4)
    assert trainer.plot_latent_interpolations(codes[:0], 'contour') == []


def test_write_measures_round_trip(dev, tmp_path, monkeypatch):
    trainer = tiny_trainer(tmp_path, monkeypatch)
    tokens = pc.measures(9, 24, seed=21)
    tokens = tokens[(tokens >= 0).all(1) & (tokens < V).all(1)][:5]        # (a vocabulary index, as a decoder returns them)
    values = np.array([-0.5, -3.25, np.nan, -0.75, -9.0], np.float32)      # log-probabilities, one missing
    mid, png = trainer.write_measures(torch.from_numpy(tokens)[:, None], str(tmp_path / 'out' / 'five'), values=values)
    assert (mid, png) == (str(tmp_path / 'out' / 'five.mid'), str(tmp_path / 'out' / 'five.png'))
    assert midi.read_midi(mid) == (480, midi_notes(tokens))
    assert np.array_equal(read_png(png), pc.pianoroll(tokens[None], MIDI_LUT, IS_NOTE, SLUR, values[None])[0])
    back = np.array(midi.tokens_from_notes(midi.read_midi(mid)[1], N2I, 5, division=480))
    assert np.array_equal(pc.events(back, MIDI_LUT, IS_NOTE, SLUR)[:, :, 0], pc.events(tokens, MIDI_LUT, IS_NOTE, SLUR)[:, :, 0])
    # an attribute's labels beside the roll; a look of the caller's; a lone measure without a panel
    mid, png = trainer.write_measures(tokens, str(tmp_path / 'attr'), attr_str='note_density', px_per_twelfth=1, px_per_pitch=2)
    labels = trainer.compute_attribute_labels(torch.from_numpy(tokens).to(dev), ['note_density']).cpu().numpy().reshape(1, 5)
    assert np.array_equal(read_png(png), pc.pianoroll(tokens[None], MIDI_LUT, IS_NOTE, SLUR, labels, px_per_twelfth=1, px_per_pitch=2)[0])
    mid, png = trainer.write_measures(tokens[0], str(tmp_path / 'one'))
    assert read_png(png).shape == (120, 96, 3) and midi.read_midi(mid) == (480, midi_notes(tokens[:1]))


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------------
def _run_cli(args, tmp_path):
    env = dict(os.environ, ARVAE_DATA_DIR=str(tmp_path), ARVAE_MODEL_DIR=str(tmp_path / 'models'))
    common = ['--batch_size', '16', '--rand', '1', '-r', 'all', '--encoder_hidden_size', '64', '--decoder_hidden_size', '64']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_measure_vae.py')] + args + common, capture_output=True, text=True,
                       timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.JSONDecoder().raw_decode(r.stdout[r.stdout.index('{\n'):])[0]


def test_cli_writes_plots_and_reads_midi(dev, tmp_path):
    """on write_folk data: a one-epoch run with --sample 2 --write_midi DIR --plots writes the files its summary lists; --infill 1
    --from_midi of one of them reproduces the kept ticks, in the rewritten measure and in the four beam alternatives written beside it"""
    write_folk(str(tmp_path), 400)
    out = tmp_path / 'heard'
    summary = _run_cli(['--num_epochs', '1', '--sample', '2', '--write_midi', str(out), '--plots'], tmp_path)
    assert summary['written'] == [str(out / f'sample_{i}{ext}') for i in range(2) for ext in ('.mid', '.png')]
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in summary['written'])
    for i, names in enumerate(summary['samples']):
        tokens = np.array([[N2I[n] for n in names]])
        assert midi.read_midi(str(out / f'sample_{i}.mid')) == (480, midi_notes(tokens))
        assert np.array_equal(read_png(str(out / f'sample_{i}.png')), pc.pianoroll(tokens[None], MIDI_LUT, IS_NOTE, SLUR)[0])
    plots = summary['plots']
    n = summary['num_codes']
    assert n == 16 and len(plots) == 4 * 3 * n and all(os.path.exists(p) for p in plots)
    folder = os.path.dirname(plots[0])
    assert folder.endswith('results') and sorted(os.listdir(folder)) == sorted(set(os.path.basename(p) for p in plots))
    for attr in ('rhy_complexity', 'pitch_range', 'note_density', 'contour'):
        assert os.path.join(folder, f'latent_interpolations_{attr}_{n - 1}.png') in plots
        png = read_png(os.path.join(folder, f'latent_interpolations_{attr}_0.png'))
        assert png.shape == (120, 548, 3)
        check_panel(png, 5)
    # a user's file: sample 0 comes back as canonical tokens, and the ticks kept of it stay
    # (searched in two beam groups: the four alternatives go into one file, their log_probs beside the roll)
    again = _run_cli(['--test', '--infill', '1', '--keep_ticks', '0-11', '--from_midi', str(out / 'sample_0.mid'), '--write_midi',
                      str(tmp_path / 'again'), '--beam', '4', '--beam_groups', '2', '--diversity', '0.5'], tmp_path)
    names = again['infill']['original'][0]
    notes = midi.read_midi(str(out / 'sample_0.mid'))[1]
    assert [N2I[x] for x in names] == midi.tokens_from_notes(notes, N2I, 1, division=480)[0]
    assert again['infill']['infilled'][0][:12] == names[:12] and len(again['infill']['infilled'][0]) == 24
    assert again['written'] == [str(tmp_path / 'again' / f'infill_0_{what}{ext}') for what in ('original', 'infilled', 'alternatives')
                                for ext in ('.mid', '.png')]
    assert midi.read_midi(again['written'][0])[1] == notes
    alt = again['infill']['alternatives'][0]
    tokens = np.array([[N2I[x] for x in m] for m in alt['measures']])
    assert tokens.shape == (4, 24) and all(m[:12] == names[:12] for m in alt['measures'])
    assert midi.read_midi(again['written'][4]) == (480, midi_notes(tokens))
    values = np.array([alt['log_probs']], np.float32)
    assert np.array_equal(read_png(again['written'][5]), pc.pianoroll(tokens[None], MIDI_LUT, IS_NOTE, SLUR, values)[0])

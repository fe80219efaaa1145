#!/usr/bin/env python3
"""Train / evaluate the MeasureVAE on MI355X: counterpart of the reference's train_measure_vae.py (same flags and
defaults).  Only the `folk` one-bar dataset in its pre-built tensor form is supported (arvae_amd.data.FolkNBarDataset):
building it from ABC files with music21, and the `bach` chorales, are offline steps outside this build.  `--metrics` adds the
reference's disentanglement metrics (arvae_amd.evaluation) to the evaluation summary; `--sample N [--temperature T] [--top_k K]
[--top_p P] [--playable]` adds N measures drawn from the model (z from the prior, every note from softmax(probs / T) over the notes a
top-k cut, a nucleus cut and the playable-note mask leave) as lists of note names; `--infill N --keep_ticks SPEC [--keep_rhythm]`
rewrites N measures of the evaluation split around the ticks SPEC keeps (MeasureVAETrainer.infill_measures); `--write_midi DIR` writes
what these two decode into DIR as MIDI files and piano-roll PNGs, `--from_midi FILE` lets `--infill` rewrite the measures of a MIDI
file, and `--plots` writes the reference's latent-interpolation MIDI files and piano rolls of every attribute
(MeasureVAETrainer.plot_latent_interpolations) into models/<repr>/results/; `--data_dist` and `--surfaces` write the scatter figures
of its commented-out blocks there, data_dist_<attr>.png and latent_surface_<attr>.png (plot_data_dist, plot_latent_surface: rendered
on the device, arvae_amd.ops.render_scatter)."""
import json
import os
import sys

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from arvae_amd.evaluation import eval_metrics_or_warn  # noqa: E402
from arvae_amd.data import FolkNBarDataset  # noqa: E402
from arvae_amd.measure_vae import MeasureVAE, check_sampling_cuts  # noqa: E402
from arvae_amd.measure_vae_trainer import MUSIC_REG_TYPE, MeasureVAETrainer  # noqa: E402


def reg_dims_for(reg_type, attr_dict):
    if len(reg_type) == 0:
        return (0,)
    if len(reg_type) == 1 and reg_type[0] == 'all':
        return tuple(attr_dict.values())
    return tuple(attr_dict[r] for r in reg_type)


# flag surface of the reference script (names, defaults and help strings are the drop-in contract), kept as a table
MEASURE_FLAGS = [
    (('--dataset_type', '-d'), dict(default='folk', help='dataset to be used, `bach` or `folk`')),
    (('--note_embedding_dim',), dict(default=10, help='size of the note embeddings')),
    (('--metadata_embedding_dim',), dict(default=2, help='size of the metadata embeddings')),
    (('--num_encoder_layers',), dict(default=2, help='number of layers in encoder RNN')),
    (('--encoder_hidden_size',), dict(default=128, help='hidden size of the encoder RNN')),
    (('--encoder_dropout_prob',), dict(default=0.5, help='float, amount of dropout prob between encoder RNN layers')),
    (('--has_metadata',), dict(default=False, help='bool, True if data contains metadata')),
    (('--latent_space_dim',), dict(default=32, help='int, dimension of latent space parameters')),
    (('--num_decoder_layers',), dict(default=2, help='int, number of layers in decoder RNN')),
    (('--decoder_hidden_size',), dict(default=128, help='int, hidden size of the decoder RNN')),
    (('--decoder_dropout_prob',), dict(default=0.5, help='float, amount got dropout prob between decoder RNN layers')),
    (('--batch_size',), dict(default=256, help='training batch size')),
    (('--num_epochs',), dict(default=30, help='number of training epochs')),
    (('--lr',), dict(default=1e-4, help='learning rate')),
    (('--beta',), dict(default=0.001, help='parameter for weighting KLD loss')),
    (('--capacity',), dict(default=0.0, help='parameter for beta-VAE capacity')),
    (('--gamma',), dict(default=1.0, help='parameter for weighting regularization loss')),
    (('--delta',), dict(default=10.0, help='parameter for controlling the spread')),
    (('--train/--test',), dict(default=True, help='train or test the specified model')),
    (('--log/--no_log',), dict(default=False, help='log the results for tensorboard')),
    (('--rand',), dict(default=None, help='random seed for the random number generator')),
    (('--reg_type', '-r'), dict(default=None, multiple=True, help='attribute name string to be used for regularization')),
]
# not in the reference script (whose evaluation always prints the metrics): opt-in here, so that the summary stays as it was.  It
# is read by run() around the reference's flag surface (main's parameters stay exactly the reference's)
METRICS_FLAG = '--metrics'
METRICS_HELP = (f'{METRICS_FLAG}: add the disentanglement metrics (Interpretability, SCC, Modularity, MIG, SAP; '
                'arvae_amd.evaluation) to the evaluation summary.')
with_metrics = False
# likewise opt-in and outside the reference's flags: measures drawn from the evaluated model (MeasureVAETrainer.sample_measures)
SAMPLE_FLAG, TEMPERATURE_FLAG = '--sample', '--temperature'
TOP_K_FLAG, TOP_P_FLAG, PLAYABLE_FLAG = '--top_k', '--top_p', '--playable'
BEAM_FLAG = '--beam'
SAMPLE_HELP = (f'{SAMPLE_FLAG} N [{TEMPERATURE_FLAG} T] [{TOP_K_FLAG} K] [{TOP_P_FLAG} P] [{PLAYABLE_FLAG}]: add `samples` to the '
               'evaluation summary, N measures drawn from the model (z from the prior, every note from softmax(probs / T), T = 1 by '
               'default) as 24 note names each; K keeps the K most likely notes, P the most likely notes up to a share P of the mass, '
               f'{PLAYABLE_FLAG} keeps START, END and None out.  These three are echoed as `sampling`.  '
               f'{SAMPLE_FLAG} N {BEAM_FLAG} W [{PLAYABLE_FLAG}]: the N prior draws are decoded by beam search over W beams instead of '
               f'drawing notes (the most likely measure of each code); not together with {TOP_K_FLAG}, {TOP_P_FLAG} or '
               f'{TEMPERATURE_FLAG}.')
num_samples, temperature, top_k, top_p, playable, beam = 0, 1.0, None, None, False, None
# infilling (MeasureVAETrainer.infill_measures): N measures of the evaluation split, decoded again around the ticks that are kept
INFILL_FLAG, KEEP_TICKS_FLAG, KEEP_RHYTHM_FLAG = '--infill', '--keep_ticks', '--keep_rhythm'
INFILL_HELP = (f'{INFILL_FLAG} N {KEEP_TICKS_FLAG} SPEC [{KEEP_RHYTHM_FLAG}]: add `infill` to the evaluation summary, the first N '
               'measures of the evaluation split and what the model writes around the ticks SPEC keeps of them (SPEC like 0-5,12-17: '
               f'ticks and inclusive ranges in [0, 23]); {KEEP_RHYTHM_FLAG} also keeps every slur where it is and every onset an onset.  '
               f'The notes are the best allowed ones, drawn with {TEMPERATURE_FLAG} / {TOP_K_FLAG} / {TOP_P_FLAG}, or searched with '
               f'{BEAM_FLAG} W; {PLAYABLE_FLAG} keeps START, END and None out of the rewritten ticks.')
num_infill, keep_ticks, keep_rhythm, drew_notes = 0, None, False, False
# diverse beam search (MeasureVAETrainer.decode_alternatives / infill_alternatives): several different measures per code
BEAM_GROUPS_FLAG, DIVERSITY_FLAG = '--beam_groups', '--diversity'
ALTERNATIVES_HELP = (f'{BEAM_FLAG} W {BEAM_GROUPS_FLAG} G {DIVERSITY_FLAG} L (both, and only with {BEAM_FLAG}; G divides W, L >= 0): the '
                     'W beams are searched in G groups, a group paying L for every note an earlier group has just taken.  '
                     f'{SAMPLE_FLAG} then adds `alternatives` to the summary and {INFILL_FLAG} to its `infill` entry: per measure the W '
                     'measures as note names, group by group and best first within a group, and their `log_probs`; `samples` / '
                     '`infilled` hold the first of them.  G and L are echoed as `beam_groups` and `diversity`.')
beam_groups, diversity = None, None
# listening and looking: MIDI files and piano-roll PNGs of what the model decodes (arvae_amd.midi, ops.render_pianoroll)
PLOTS_FLAG, WRITE_MIDI_FLAG, FROM_MIDI_FLAG = '--plots', '--write_midi', '--from_midi'
FILES_HELP = (f'{PLOTS_FLAG}: for every attribute and the first 20 evaluation codes write original_{{i}}.mid, '
              'latent_interpolations_{attr}_{i}.mid and the piano roll latent_interpolations_{attr}_{i}.png into models/<repr>/results/ '
              f'(listed as `plots` in the summary).  {WRITE_MIDI_FLAG} DIR: write what {SAMPLE_FLAG} and {INFILL_FLAG} decode into DIR, one '
              '.mid and one .png each: the samples, the original and the rewritten measures, and the beam alternatives with their '
              f'log_probs beside the roll (listed as `written`).  {FROM_MIDI_FLAG} FILE: {INFILL_FLAG} N rewrites the first N measures of '
              'a monophonic MIDI file on the 24-tick grid instead of the evaluation split; the file has as many measures of 4/4 as its '
              'track is long, silent ones included.')
with_plots, midi_dir, from_midi = False, None, None
# the latent plane (MeasureVAETrainer.plot_data_dist / plot_latent_surface): the reference script's commented-out blocks
DATA_DIST_FLAG, SURFACES_FLAG = '--data_dist', '--surfaces'
PLANE_HELP = (f'{DATA_DIST_FLAG}: for every attribute write data_dist_{{attr}}.png into models/<repr>/results/, the codes of the test '
              'split (batches of 128, at most 100 of them) in the plane of the attribute\'s dimension of the interpretability metric '
              f'and the last dimension that belongs to no attribute, coloured by the attribute (listed as `data_dist`).  {SURFACES_FLAG}: '
              'write latent_surface_{attr}.png of every attribute over the same planes at a grid step of 0.05, each plane decoded '
              'once for all attributes (listed as `surfaces`).')
with_data_dist, with_surfaces = False, False
TICKS = 24


def parse_keep_ticks(spec):
    """'0-5,12-17' -> a list of 24 flags: comma-separated ticks and inclusive ranges lo-hi in [0, 23], at least one tick"""
    keep = [False] * TICKS
    parts = [p.strip() for p in str(spec).split(',')]
    if not spec or any(not p for p in parts):
        raise ValueError(f'{KEEP_TICKS_FLAG} takes ticks and ranges like 0-5,12-17, got {spec!r}')
    for part in parts:
        ends = part.split('-')
        if len(ends) > 2 or not all(e.strip().isdigit() for e in ends):
            raise ValueError(f'{KEEP_TICKS_FLAG}: {part!r} is neither a tick nor a range lo-hi (in {spec!r})')
        lo, hi = int(ends[0]), int(ends[-1])
        if lo > hi:
            raise ValueError(f'{KEEP_TICKS_FLAG}: the range {part!r} runs backwards')
        if hi >= TICKS:
            raise ValueError(f'{KEEP_TICKS_FLAG}: {part!r} is outside the measure\'s ticks [0, {TICKS - 1}]')
        for t in range(lo, hi + 1):
            keep[t] = True
    return keep


def with_options(fn):
    for names, kwargs in reversed(MEASURE_FLAGS):
        fn = click.option(*names, **kwargs)(fn)
    return click.command(epilog='  '.join((METRICS_HELP, SAMPLE_HELP, INFILL_HELP, ALTERNATIVES_HELP, FILES_HELP, PLANE_HELP)))(fn)


@with_options
def main(dataset_type, note_embedding_dim, metadata_embedding_dim, num_encoder_layers, encoder_hidden_size,
         encoder_dropout_prob, latent_space_dim, num_decoder_layers, decoder_hidden_size, decoder_dropout_prob,
         has_metadata, batch_size, num_epochs, lr, beta, capacity, gamma, delta, train, log, rand, reg_type):
    if dataset_type == 'folk':
        dataset = FolkNBarDataset(dataset_type='train', is_short=False, num_bars=1)
    elif dataset_type == 'bach':
        raise SystemExit('the `bach` chorale dataset needs music21 preprocessing, which is outside this build')
    else:
        raise ValueError('Invalid dataset_type. Choose between `folk` and `bach`')
    reg_dim = reg_dims_for(reg_type, MUSIC_REG_TYPE)
    seeds = range(0, 10) if rand is None else [int(rand)]
    # launched by torch.distributed.run: one process per GPU, minibatch rows sharded over the ranks, gradients all-reduced
    # over RCCL (arvae_amd.parallel); --batch_size is then the per-GPU batch
    from arvae_amd.parallel import init_from_env
    dp = init_from_env() if train else None
    chief = dp is None or dp.rank == 0

    def build(seed):
        # the reference builds the model BEFORE the trainer seeds torch (train_image_vae.py:97-109, image_vae_trainer.py:103):
        # its initial weights differ from run to run.  Here the run's seed covers them too (same run, same weights)
        torch.manual_seed(seed)
        model = MeasureVAE(dataset=dataset, note_embedding_dim=note_embedding_dim,
                           metadata_embedding_dim=metadata_embedding_dim, num_encoder_layers=num_encoder_layers,
                           encoder_hidden_size=encoder_hidden_size, encoder_dropout_prob=encoder_dropout_prob,
                           latent_space_dim=latent_space_dim, num_decoder_layers=num_decoder_layers,
                           decoder_hidden_size=decoder_hidden_size, decoder_dropout_prob=decoder_dropout_prob,
                           has_metadata=has_metadata, dataset_type=dataset_type)
        trainer = MeasureVAETrainer(dataset=dataset, model=model, lr=lr, reg_type=reg_type, reg_dim=reg_dim, beta=beta,
                                    capacity=capacity, gamma=gamma, delta=delta, rand=seed)
        return model, trainer

    # every rank trains every seed first; rank 0 evaluates afterwards, once the process group is gone -- a rank that waits in
    # a pending RCCL collective while rank 0 evaluates would be killed by the group's watchdog timeout (advisor, round 2)
    if train:
        if not torch.cuda.is_available():
            raise SystemExit('training needs a GPU: the AR-VAE path has no CPU fallback')
        try:
            for seed in seeds:
                model, trainer = build(seed)
                trainer.cuda()
                if dp is not None:
                    dp.attach(trainer)
                trainer.train_model(batch_size=batch_size, num_epochs=num_epochs, log=log)
                trainer.data_parallel = None
            if dp is not None:
                dp.finish()
        except BaseException:
            # a rank that fails must not leave its peers waiting in a collective: give the communicator up without waiting for
            # them (ncclCommAbort) and let the error end this process non-zero -- the launcher then ends the other ranks, whose
            # own bounded waits (parallel.LibraryComm.wait_idle) raise in the meantime
            if dp is not None:
                dp.abort()
            raise
    if not chief:
        return
    for seed in seeds:
        model, trainer = build(seed)
        trainer.load_model()
        trainer.writer = None
        eval_bs = min(256, batch_size)                  # the reference evaluates with 256; smaller runs keep their own size
        _, _, eval_loader = dataset.data_loaders(batch_size=eval_bs)
        codes, attrs, names = trainer.compute_representations(eval_loader)
        summary = {'model': repr(model), 'num_codes': int(codes.shape[0]), 'attributes': names,
                   'attribute_means': [float(v) for v in attrs.mean(0)]}
        summary.update(trainer.test_model(batch_size=eval_bs))
        with_plane = with_data_dist or with_surfaces
        metrics = eval_metrics_or_warn(codes, attrs, names) if with_metrics or with_plots or with_plane else {}      # (once, for all of them)
        if with_metrics:
            summary.update(metrics)
        written = []
        if num_samples > 0:
            trainer.cuda()
            model.eval()
            if beam_groups is not None:
                from arvae_amd import ops
                z = ops.normal_noise((num_samples, latent_space_dim), next(model.parameters()).device)
                seqs, log_probs = trainer.decode_alternatives(z, beam, beam_groups, diversity, playable=playable)
                notes = seqs[:, :1]
                summary['alternatives'] = _alternatives(dataset.index2note_dicts, seqs, log_probs)
            else:
                _, notes = trainer.sample_measures(num_samples, temperature, top_k=top_k, top_p=top_p, playable=playable, beam_width=beam)
            if beam_groups is not None:
                summary['sampling'] = {'beam': beam, 'beam_groups': beam_groups, 'diversity': diversity, 'playable': playable}
            elif beam is not None:
                summary['sampling'] = {'beam': beam, 'playable': playable}
            elif top_k is not None or top_p is not None or playable:        # the cuts are echoed beside the measures they shaped
                summary['sampling'] = {'temperature': temperature, 'top_k': top_k, 'top_p': top_p, 'playable': playable}
            summary['samples'] = [[dataset.index2note_dicts[int(i)] for i in row] for row in notes.squeeze(1).tolist()]
            if midi_dir is not None:
                for i in range(num_samples):
                    written += trainer.write_measures(notes[i], os.path.join(midi_dir, f'sample_{i}'))
                    if beam_groups is not None:
                        written += trainer.write_measures(seqs[i], os.path.join(midi_dir, f'sample_{i}_alternatives'), values=log_probs[i])
        if num_infill > 0:
            trainer.cuda()
            model.eval()
            if from_midi is not None:
                score = measures_of_midi(from_midi, dataset.note2index_dicts)[:num_infill]
                if score.shape[0] < num_infill:
                    raise SystemExit(f'{INFILL_FLAG} {num_infill}: {from_midi} holds {score.shape[0]} measures')
            else:
                score = next(iter(eval_loader))[0]
                score = score.view(-1, score.shape[-1])[:num_infill]
                if score.shape[0] < num_infill:
                    raise SystemExit(f'{INFILL_FLAG} {num_infill}: an evaluation batch holds {score.shape[0]} measures')
            mode = 'beam' if beam is not None else ('multinomial' if drew_notes else 'argmax')
            keep = None if keep_ticks is None else torch.tensor(keep_ticks)
            if beam_groups is not None:
                seqs, log_probs = trainer.infill_alternatives(score, keep=keep, keep_rhythm=keep_rhythm, playable=playable, beam_width=beam,
                                                              beam_groups=beam_groups, diversity=diversity)
                notes = seqs[:, :1]
            else:
                _, notes = trainer.infill_measures(score, keep=keep, keep_rhythm=keep_rhythm, sampling=mode, temperature=temperature,
                                                   top_k=top_k, top_p=top_p, playable=playable, beam_width=4 if beam is None else beam)
            names = dataset.index2note_dicts
            summary['infill'] = {'sampling': mode, 'keep_ticks': [t for t in range(TICKS) if keep_ticks is not None and keep_ticks[t]],
                                 'keep_rhythm': keep_rhythm, 'playable': playable,
                                 'original': [[names[int(i)] for i in row] for row in score.tolist()],
                                 'infilled': [[names[int(i)] for i in row] for row in notes.squeeze(1).tolist()]}
            if beam_groups is not None:
                summary['infill'].update(beam_groups=beam_groups, diversity=diversity, alternatives=_alternatives(names, seqs, log_probs))
            if midi_dir is not None:
                for i in range(num_infill):
                    written += trainer.write_measures(score[i], os.path.join(midi_dir, f'infill_{i}_original'))
                    written += trainer.write_measures(notes[i], os.path.join(midi_dir, f'infill_{i}_infilled'))
                    if beam_groups is not None:
                        written += trainer.write_measures(seqs[i], os.path.join(midi_dir, f'infill_{i}_alternatives'), values=log_probs[i])
        if midi_dir is not None:
            summary['written'] = written
        if with_plots:
            if 'interpretability' not in metrics:
                print(f'{PLOTS_FLAG}: the figures sweep the dimensions of the interpretability metric, which this evaluation split '
                      f'({codes.shape[0]} codes) was too small to compute; skipped')
            else:
                trainer.cuda()
                model.eval()
                trainer.metrics = dict(metrics)
                summary['plots'] = []
                for attr_str in trainer.attr_dict:           # the reference script's live loop (train_measure_vae.py:199-211)
                    summary['plots'] += trainer.plot_latent_interpolations(codes, attr_str=attr_str, num_points=20)
        if with_plane and 'interpretability' not in metrics:
            print(f'{DATA_DIST_FLAG} / {SURFACES_FLAG}: the planes are those of the interpretability metric\'s dimensions, which this '
                  f'evaluation split ({codes.shape[0]} codes) was too small to compute; skipped')
        elif with_plane:
            # the reference script's commented-out blocks (train_measure_vae.py:188-210): the attribute's dimension against the last
            # dimension that belongs to no attribute
            trainer.cuda()
            model.eval()
            attr_names = list(trainer.attr_dict)
            attr_dims = [int(metrics['interpretability'][a][0]) for a in attr_names]
            other = [d for d in range(latent_space_dim) if d not in attr_dims][-1]
            if with_data_dist:
                _, _, loader = dataset.data_loaders(batch_size=min(128, batch_size))
                dist_codes, dist_attrs, _ = trainer.compute_representations(loader, num_batches=min(100, len(loader)))
                summary['data_dist'] = trainer.plot_data_dist(dist_codes, dist_attrs, attr_names, attr_dims, other)
            if with_surfaces:
                summary['surfaces'] = trainer.plot_latent_surface(attr_names, attr_dims, other, grid_res=0.05)
        print(json.dumps(summary, indent=2))


def measures_of_midi(path, note2index):
    """the measures of a monophonic MIDI file on the 24-tick grid as canonical tokens, (measures, 24) int64 (arvae_amd.midi)"""
    from arvae_amd import midi
    division, notes, length = midi.read_midi(path, with_length=True)       # (the track's length: silent measures at the end count)
    count = max(1, -(-max([length] + [on + dur for on, dur, _ in notes]) // (4 * division)))
    return torch.tensor(midi.tokens_from_notes(notes, note2index, count, division=division), dtype=torch.int64)


def _alternatives(names, seqs, log_probs):
    """the summary's form of decode_alternatives' result: per measure its W measures as names and their log_probs"""
    return [{'measures': [[names[int(i)] for i in row] for row in code], 'log_probs': [float(x) for x in lp]}
            for code, lp in zip(seqs.tolist(), log_probs.tolist())]


def _take_value(argv, flag, cast, default):
    """-> (value of `flag VALUE` / `flag=VALUE` in argv or default, argv without it)"""
    rest, value, i = [], default, 0
    while i < len(argv):
        a = argv[i]
        if a == flag:
            if i + 1 >= len(argv):
                raise SystemExit(f'{flag} needs a value')
            value, i = cast(argv[i + 1]), i + 1
        elif a.startswith(flag + '='):
            value = cast(a[len(flag) + 1:])
        else:
            rest.append(a)
        i += 1
    return value, rest


def run(argv=None):
    """the command line: the reference's flags (main) plus this build's opt-in --metrics, --sample, --temperature, --top_k, --top_p,
    --playable, --beam, --beam_groups / --diversity, --infill, --plots, --write_midi, --from_midi, --data_dist and --surfaces.  Values of --top_k / --top_p outside their ranges raise the decoder's
    ValueError (sampling_filter); --beam takes a width in [1, 16] and is refused together with --top_k, --top_p or --temperature
    (beam search draws nothing); --beam_groups and --diversity come together and only with --beam."""
    global with_metrics, num_samples, temperature, top_k, top_p, playable, beam, num_infill, keep_ticks, keep_rhythm, drew_notes
    global beam_groups, diversity, with_plots, midi_dir, from_midi, with_data_dist, with_surfaces
    argv = sys.argv[1:] if argv is None else list(argv)
    with_metrics = METRICS_FLAG in argv
    with_plots = PLOTS_FLAG in argv
    with_data_dist, with_surfaces = DATA_DIST_FLAG in argv, SURFACES_FLAG in argv
    midi_dir, argv = _take_value(argv, WRITE_MIDI_FLAG, str, None)
    from_midi, argv = _take_value(argv, FROM_MIDI_FLAG, str, None)
    playable = PLAYABLE_FLAG in argv
    num_samples, argv = _take_value(argv, SAMPLE_FLAG, int, 0)
    drew = any(a == TEMPERATURE_FLAG or a.startswith(TEMPERATURE_FLAG + '=') for a in argv)
    temperature, argv = _take_value(argv, TEMPERATURE_FLAG, float, 1.0)
    top_k, argv = _take_value(argv, TOP_K_FLAG, int, None)
    top_p, argv = _take_value(argv, TOP_P_FLAG, float, None)
    beam, argv = _take_value(argv, BEAM_FLAG, int, None)
    if beam is not None:
        if not 1 <= beam <= 16:
            raise ValueError(f'{BEAM_FLAG} takes a beam width in [1, 16], got {beam}')
        if top_k is not None or top_p is not None or drew:
            raise ValueError(f'{BEAM_FLAG} decodes by beam search, which draws no note: it cannot be combined with {TOP_K_FLAG}, '
                             f'{TOP_P_FLAG} or {TEMPERATURE_FLAG}')
    beam_groups, argv = _take_value(argv, BEAM_GROUPS_FLAG, int, None)
    diversity, argv = _take_value(argv, DIVERSITY_FLAG, float, None)
    if beam_groups is not None or diversity is not None:       # refused here, before anything is loaded
        if beam is None:
            raise ValueError(f'{BEAM_GROUPS_FLAG} and {DIVERSITY_FLAG} group the beams of {BEAM_FLAG} W: give {BEAM_FLAG}')
        if beam_groups is None or diversity is None:
            raise ValueError(f'{BEAM_GROUPS_FLAG} G and {DIVERSITY_FLAG} L are given together')
        if not 1 <= beam_groups <= beam or beam % beam_groups:
            raise ValueError(f'{BEAM_GROUPS_FLAG} takes a count in [1, {beam}] that divides {BEAM_FLAG} {beam}, got {beam_groups}')
        if not (diversity >= 0 and diversity != float('inf')):
            raise ValueError(f'{DIVERSITY_FLAG} takes a finite number >= 0, got {diversity}')
    num_infill, argv = _take_value(argv, INFILL_FLAG, int, 0)
    spec, argv = _take_value(argv, KEEP_TICKS_FLAG, str, None)
    keep_rhythm = KEEP_RHYTHM_FLAG in argv
    keep_ticks = None if spec is None else parse_keep_ticks(spec)      # a bad spec is refused here, before anything is loaded
    drew_notes = drew or top_k is not None or top_p is not None
    if num_infill < 0:
        raise ValueError(f'{INFILL_FLAG} takes a count >= 0, got {num_infill}')
    if num_infill > 0 and keep_ticks is None and not keep_rhythm:
        raise ValueError(f'{INFILL_FLAG} keeps something of every measure: give {KEEP_TICKS_FLAG} SPEC or {KEEP_RHYTHM_FLAG}')
    if num_infill == 0 and (keep_ticks is not None or keep_rhythm):
        raise ValueError(f'{KEEP_TICKS_FLAG} and {KEEP_RHYTHM_FLAG} belong to {INFILL_FLAG} N')
    if midi_dir is not None and num_infill == 0 and num_samples <= 0:
        raise ValueError(f'{WRITE_MIDI_FLAG} writes what {SAMPLE_FLAG} N and {INFILL_FLAG} N decode: give one of them')
    if from_midi is not None and num_infill == 0:
        raise ValueError(f'{FROM_MIDI_FLAG} gives {INFILL_FLAG} N its measures: give {INFILL_FLAG}')
    if from_midi is not None and not os.path.isfile(from_midi):
        raise ValueError(f'{FROM_MIDI_FLAG}: no file {from_midi}')
    if num_samples < 0 or not temperature > 0:
        raise SystemExit(f'{SAMPLE_FLAG} takes a count >= 0 and {TEMPERATURE_FLAG} a positive number')
    check_sampling_cuts(top_k, top_p)          # the decoder's own ValueError, before anything is loaded or trained
    main(args=[a for a in argv if a not in (METRICS_FLAG, PLAYABLE_FLAG, KEEP_RHYTHM_FLAG, PLOTS_FLAG, DATA_DIST_FLAG, SURFACES_FLAG)])


if __name__ == '__main__':
    run()

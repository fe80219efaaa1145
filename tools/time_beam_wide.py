"""Time of MeasureVAE's beam search at the hidden sizes of csrc/beam_wide.hip, B = 256, timed with device events after a warm-up, at
the two configurations of tools/time_tick_wide.py
    default   the class's own: encoder 512, decoder 512, latent 256
    h256      encoder 256, decoder 256, latent 32
three workloads per configuration
    beam4     decoder.beam_search of B codes, width 4
    groups    decoder.beam_search of B codes, width 8 in 4 groups at diversity 0.5 under the trainer's playable mask
    infill    trainer.infill_measures of B measures, ticks 0-5 and 12-17 kept, sampling='beam', width 4
for up to three builds that ALTERNATE inside every repeat on the same device:
    parent    --parent-root: a checkout of the parent commit with its library built (the search runs tick by tick there)
    new       this tree: one arvae_tick_beam_search_wide* call per search
    stepwise  this tree with ARVAE_TICK_STEPWISE=1: the same code as the parent's path, a cross-check of the comparison itself
Every (build, repeat) is one fresh child process that times the six (configuration, workload) pairs; the parent process never opens
the GPU.  Per pair the medians of all repeats are printed, the spread (max - min) of the repeated parent runs, and whether the new
path is faster than the parent by more than that spread.  Beside the times: library calls per search -- torch's own kernels are not
among them, and a call that issues several launches counts once.

    python tools/time_beam_wide.py [--parent-root /path/to/parent] [--repeats 3] [--steps 10] [--warmup 3]
"""
import argparse, json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {'default': (512, 512, 256), 'h256': (256, 256, 32)}
PAIRS = [(c, m) for c in CONFIGS for m in ('beam4', 'groups', 'infill')]

ap = argparse.ArgumentParser()
ap.add_argument('--parent-root', default=None)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batch', type=int, default=256)
ap.add_argument('--worker', default=None, help='internal: the tree whose package this process times')
args = ap.parse_args()


def worker(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from arvae_amd import _lib, synthetic as syn
    from arvae_amd.measure_vae import MeasureVAE
    from arvae_amd.measure_vae_trainer import MeasureVAETrainer

    class FolkDataset:
        class_name, n_bars = '4by4_FolkNBarDataset_1_', 1

        def __init__(self):
            self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

        def __repr__(self):
            return self.class_name

    lib = _lib.load()
    count = {'calls': 0}

    def counted(fn):
        def call(*a):
            count['calls'] += 1
            return fn(*a)
        return call

    for name in _lib.SIGNATURES:
        if name.endswith(('_supported', '_ws_floats', '_ws_bytes', '_fits')) or name in ('arvae_abi_version', 'arvae_last_error_string'):
            continue
        setattr(lib, name, counted(getattr(lib, name)))
    dev = torch.device('cuda:0')
    score = syn.measure_batch(args.batch, seed=18)
    keep = np.zeros(24, bool)
    keep[:6] = keep[12:18] = True
    out = {}
    for cfg in CONFIGS:
        enc, dec, z = CONFIGS[cfg]
        torch.manual_seed(11)
        ds = FolkDataset()
        model = MeasureVAE(ds, 10, 2, 2, enc, 0.5, z, 2, dec, 0.5, False, 'folk')
        trainer = MeasureVAETrainer(ds, model, lr=1e-4, reg_type=('all',), reg_dim=(0, 1, 2, 3), beta=0.001, gamma=1.0, capacity=0.0,
                                    rand=0, delta=10.0)
        trainer.cuda()
        model.eval()
        codes = torch.from_numpy(syn.normal_noise((args.batch, z), seed=19)).to(dev)
        playable = trainer.playable_mask()

        def beam4():
            model.decoder.beam_search(codes, 4)

        def groups():
            model.decoder.beam_search(codes, 8, allowed=playable, beam_groups=4, diversity=0.5)

        def infill():
            trainer.infill_measures(score, keep=keep, sampling='beam', beam_width=4)

        for mode, run in (('beam4', beam4), ('groups', groups), ('infill', infill)):
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            count['calls'] = 0
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for e0, e1 in ev:
                e0.record()
                run()
                e1.record()
            torch.cuda.synchronize()
            out[f'{cfg}/{mode}'] = {'ms': round(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev), 4),
                                    'library_calls': count['calls'] / args.steps}
        del trainer, model
    print('RESULT ' + json.dumps(out))


if args.worker is not None:
    worker(args.worker)
    sys.exit(0)

builds = ([('parent', args.parent_root, '0')] if args.parent_root else []) + [('new', HERE, '0'), ('stepwise', HERE, '1')]
runs = {name: [] for name, _, _ in builds}
for rep in range(args.repeats):                                  # the builds alternate inside a repeat: drift hits all alike
    for name, root, stepwise in builds:
        env = dict(os.environ, ARVAE_TICK_STEPWISE=stepwise)
        env.pop('ARVAE_LIB', None)
        env.pop('ARVAE_GRU_STEPWISE', None)
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', root, '--steps', str(args.steps), '--warmup', str(args.warmup),
               '--batch', str(args.batch)]
        p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:                                    # a failed child ends the run: nothing more is started on the device
            sys.stderr.write(p.stderr[-4000:])
            sys.exit(f'{name} (repeat {rep}) ended with status {p.returncode}')
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
        runs[name].append(json.loads(line[7:]))
        print(f'repeat {rep} {name}: ' + '  '.join(f'{k} {v["ms"]:.3f} ms' for k, v in runs[name][-1].items()), flush=True)

summary = {'batch': args.batch, 'steps': args.steps, 'repeats': args.repeats, 'pairs': {}}
for cfg, mode in PAIRS:
    key = f'{cfg}/{mode}'
    row = {}
    for name in runs:
        ms = [r[key]['ms'] for r in runs[name]]
        row[name] = {'ms': ms, 'median_ms': statistics.median(ms), 'spread_ms': round(max(ms) - min(ms), 4),
                     'library_calls': runs[name][-1][key]['library_calls']}
    if 'parent' in row:
        gain = row['parent']['median_ms'] - row['new']['median_ms']
        row['gain_ms'] = round(gain, 4)
        row['parent_over_new'] = round(row['parent']['median_ms'] / row['new']['median_ms'], 3)
        row['faster_by_more_than_the_parent_spread'] = bool(gain > row['parent']['spread_ms'] and max(row['new']['ms']) < min(row['parent']['ms']))
    summary['pairs'][key] = row
print(json.dumps(summary))

"""Time of one piano-roll render (ops.render_pianoroll, csrc/pianoroll.hip) for the figures of one plot_latent_interpolations call at
the command line's size -- 20 figures of 5 measures with their attribute panel, 20 x 120 x 548 x 3 bytes -- beside the numpy
restatement of tests/pianoroll_cases.py run on the host from the copied tokens.
  render: the launch alone between HIP events; launch + the copy of the uint8 frames to the host on a host clock; the events
  launch (ops.measure_notes, 100 measures) + its copy likewise;
  host: tokens and values copied to the host, then pianoroll_cases.pianoroll: host clock around the whole.
Median over --calls calls after a warm-up, --repeats times, the two alternating inside a repeat.

    python tools/time_pianoroll.py [--calls 50] [--repeats 5]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from arvae_amd import ops
import pianoroll_cases as pc

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=50)
ap.add_argument('--repeats', type=int, default=5)
args = ap.parse_args()
dev = torch.device('cuda:0')
F, K, T = 20, 5, 24
_, _, midi_lut, is_note, slur, _ = pc.vocabulary()
tables = (torch.from_numpy(midi_lut).to(dev), torch.from_numpy(is_note).to(dev))
score = torch.from_numpy(pc.random_measures(F * K, T, seed=0).reshape(F, K, T)).to(dev)
values = torch.rand(F, K, generator=torch.Generator().manual_seed(0)).to(dev)


def launch_event_us():
    out = torch.empty(F, *ops.pianoroll_geometry(K, T, True), 3, dtype=torch.uint8, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for _ in range(10):
        ops.render_pianoroll(score, tables, values, 0.0, 1.0, slur=slur, out=out)
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        ops.render_pianoroll(score, tables, values, 0.0, 1.0, slur=slur, out=out)
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def host_us(fn, calls):
    for _ in range(2):
        fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


def new():
    return ops.render_pianoroll(score, tables, values, 0.0, 1.0, slur=slur).cpu().numpy()


def events():
    return ops.measure_notes(score.view(F * K, T), tables, slur=slur).cpu().numpy()


def host():
    return pc.pianoroll(score.cpu().numpy(), midi_lut, is_note, slur, values.cpu().numpy(), 0.0, 1.0)


a, b = new(), host()
out = {'calls': args.calls, 'repeats': args.repeats, 'frame_bytes': int(a.size), 'differing_bytes': int((a != b).sum())}
assert a.shape == b.shape == (F, 120, 548, 3)
for r in range(args.repeats):
    out.setdefault('render_launch_us', []).append(round(launch_event_us(), 2))
    out.setdefault('render_to_host_us', []).append(round(host_us(new, args.calls), 1))
    out.setdefault('events_to_host_us', []).append(round(host_us(events, args.calls), 1))
    out.setdefault('numpy_on_host_us', []).append(round(host_us(host, max(3, args.calls // 10)), 1))
for key in [k for k in out if k.endswith('_us')]:
    out[key + '_median'] = statistics.median(out[key])
    out[key + '_spread'] = round(max(out[key]) - min(out[key]), 2)
print(json.dumps(out))

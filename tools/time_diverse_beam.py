"""Time of the diverse beam search (csrc/beam_decoder.hip, tick_beam_search_kernel<.., TickBeamGroups>: the W beams in G groups served
in order, include/arvae_hip.h "Diverse beam search") beside the search it extends: B = 256, H = 128, 4 beats x 6 ticks, vocabulary 35,
two layers, W = 8, G = 4, penalty 0.5.
  library level: one call = the two weight prep launches + the search kernel, HIP events around every call, median over --launches
  calls after a warm-up, --repeats times, the calls alternating inside a repeat: the ungrouped search (arvae_tick_beam_search, W = 8),
  the planned one on a plan of ones, the grouped one;
  decoder level: HierarchicalDecoder.beam_search(beam_groups=G, diversity=L) (beat RNN, the search, the whole-sequence pass on the best
  beam), host timer around a synchronised call, in one launch and tick by tick (ARVAE_TICK_STEPWISE=1: per tick the dense launches,
  the gate launches, arvae_beam_select_groups and the gathers), alternating inside a repeat.
--other-lib takes another build of the library (the parent commit's) for the ungrouped search: the existing instantiation of two
builds is compared in one run, alternately, on the same device; `spread` is the largest minus the smallest of a build's repeats.

    python tools/time_diverse_beam.py [--other-lib path/to/libarvae_hip.so] [--launches 40] [--repeats 5]
"""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from arvae_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--other-lib', default=None)
ap.add_argument('--launches', type=int, default=40)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--width', type=int, default=8)
ap.add_argument('--groups', type=int, default=4)
ap.add_argument('--penalty', type=float, default=0.5)
args = ap.parse_args()
lib = _lib.load()
other = ctypes.CDLL(args.other_lib) if args.other_lib else None
dev = torch.device('cuda:0')
B, H, V, beats, tpb, W, G = 256, 128, 35, 4, 6, args.width, args.groups
T = beats * tpb
g = torch.Generator(device='cpu').manual_seed(1)
def rnd(*shape, s=0.1): return (torch.randn(*shape, generator=g) * s).to(dev)
weights = (rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(V, H, s=0.5), rnd(V))
h0a, h0b = torch.tanh(rnd(beats * B, H, s=1.0)), torch.tanh(rnd(beats * B, H, s=1.0))
gib, ptab = rnd(beats * B, 3 * H, s=0.5), rnd(V + 1, 3 * H, s=0.5)
ones = torch.ones(V, dtype=torch.uint8, device=dev)
parents = torch.empty(B, T, W, dtype=torch.int32, device=dev)
tokens = torch.empty(B, T, W, dtype=torch.int64, device=dev)
hist = torch.empty(B, T, W, dtype=torch.float32, device=dev)
seqs = torch.empty(B, W, T, dtype=torch.int64, device=dev)
scores, logp = torch.empty(B, W, dtype=torch.float32, device=dev), torch.empty(B, W, dtype=torch.float32, device=dev)
ws = torch.empty(lib.arvae_tick_beam_search_ws_floats(H), dtype=torch.float32, device=dev)
p = lambda t: ctypes.c_void_p(t.data_ptr())
tw = _lib.TickWeights(*[p(t) for t in weights])
head = [ctypes.byref(tw), p(h0a), p(h0b), ctypes.c_int64(0), p(gib), p(ptab)] + [ctypes.c_int32(v) for v in (B, beats, tpb, H, V, W)]
outs = [p(parents), p(tokens), p(hist), p(seqs), p(scores)]
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
npl = _lib.NotePlan(p(ones), 0, 0)                              # every note, as the Python layer gives it: both strides 0
if other is not None:
    other.arvae_tick_beam_search.argtypes = lib.arvae_tick_beam_search.argtypes
calls = {'beam': lambda: lib.arvae_tick_beam_search(*head, None, ctypes.c_int32(V), *outs, p(ws), stream),
         'planned': lambda: lib.arvae_tick_beam_search_planned(*head, ctypes.byref(npl), *outs, p(ws), stream),
         'groups': lambda: lib.arvae_tick_beam_search_groups(*head, ctypes.c_int32(G), ctypes.c_float(args.penalty), ctypes.byref(npl), *outs,
                                                             p(logp), p(ws), stream)}
if other is not None:
    calls['beam_other_lib'] = lambda: other.arvae_tick_beam_search(*head, None, ctypes.c_int32(V), *outs, p(ws), stream)


def median_us(launch):
    for _ in range(10):
        assert launch() == 0
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    for e0, e1 in ev:
        e0.record()
        assert launch() == 0
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


out = {'launches': args.launches, 'width': W, 'groups': G, 'penalty': args.penalty, 'other_lib': args.other_lib}
for r in range(args.repeats):                                   # the calls alternate inside a repeat: drift hits all alike
    for name, launch in calls.items():
        out.setdefault(name + '_us', []).append(round(median_us(launch), 2))
for name in calls:
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
    out[name + '_spread_us'] = round(max(out[name + '_us']) - min(out[name + '_us']), 2)
assert calls['groups']() == 0                                   # (the last timed launch may have been another call)
torch.cuda.synchronize()
wg = W // G
assert bool(torch.isfinite(scores).all()) and bool((parents // wg == torch.arange(W, device=dev) // wg).all())
assert bool((scores <= logp).all()) and bool((scores[:, :wg] == logp[:, :wg]).all())

# HierarchicalDecoder.beam_search in groups: one launch against tick by tick
from arvae_amd.measure_vae import HierarchicalDecoder
torch.manual_seed(0)
dec = HierarchicalDecoder(10, V, 32, 2, H, 0.0).to(dev).eval()
z = rnd(B, 32, s=1.0)
configs = {'beam_search_groups_one_launch': '0', 'beam_search_groups_tick_by_tick': '1'}


def search_us(mode, n):
    os.environ['ARVAE_TICK_STEPWISE'] = mode
    run = lambda: dec.beam_search(z, W, beam_groups=G, diversity=args.penalty)
    for _ in range(3):
        run()
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


for r in range(args.repeats):
    for name, mode in configs.items():
        out.setdefault(name + '_us', []).append(round(search_us(mode, 5 if mode == '1' else 20), 1))
for name in configs:
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
    out[name + '_spread_us'] = round(max(out[name + '_us']) - min(out[name + '_us']), 1)
print(json.dumps(out))

"""Time of decoding under a note plan (csrc/tick_decoder.hip, PICK_PLANNED: the allowed notes per (row, tick)) beside the filtered draw
it extends: B = 256, H = 128, 4 beats x 6 ticks, vocabulary 35, two layers, no dropout (generation).
  library level: one call = the two weight prep launches + the tick kernel, HIP events around every call, median over --launches calls
  after a warm-up, --repeats times, the picks alternating inside a repeat (tools/time_tick_filter.py's method);
  decoder level: HierarchicalDecoder.generate (beat RNN, the free run, the whole-sequence pass on its tokens), host timer around a
  synchronised call, in three configurations that alternate inside a repeat: filtered without a plan, with a plan on the one-launch
  kernel, with a plan tick by tick (ARVAE_TICK_STEPWISE=1: per tick the dense launches, the gate launches and
  arvae_row_sample_planned).
--other-lib takes another build of the library (the parent commit's) for the filtered and the argmax pass: the existing
instantiations of two builds are compared in one run, alternately, on the same device.

    python tools/time_note_plan.py [--other-lib path/to/libarvae_hip.so] [--launches 60] [--repeats 5]
"""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from arvae_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--other-lib', default=None)
ap.add_argument('--launches', type=int, default=60)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--top_k', type=int, default=4)
ap.add_argument('--top_p', type=float, default=0.9)
args = ap.parse_args()
lib = _lib.load()
other = ctypes.CDLL(args.other_lib) if args.other_lib else None
dev = torch.device('cuda:0')
B, H, V, beats, tpb = 256, 128, 35, 4, 6
T = beats * tpb
g = torch.Generator(device='cpu').manual_seed(1)
def rnd(*shape, s=0.1): return (torch.randn(*shape, generator=g) * s).to(dev)
weights = (rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(V, H, s=0.5), rnd(V))
h0a, h0b = torch.tanh(rnd(beats * B, H, s=1.0)), torch.tanh(rnd(beats * B, H, s=1.0))
gib, ptab = rnd(beats * B, 3 * H, s=0.5), rnd(V + 1, 3 * H, s=0.5)
u = torch.rand(B, T, generator=g).clamp_(min=2.0 ** -32).to(dev)
allow = torch.ones(V, dtype=torch.uint8)
allow[[1, 2, 4]] = 0                                            # START, END and None of the folk vocabulary
# the plan: per (row, tick) free (the playable notes), forced (one note) or a subset of half the notes, a third each
rs = np.random.RandomState(101)
kinds = rs.randint(0, 3, size=(B, T))
plan_np = np.zeros((B, T, V), np.uint8)
for b in range(B):
    for t in range(T):
        if kinds[b, t] == 0:
            plan_np[b, t] = allow.numpy()
        elif kinds[b, t] == 1:
            plan_np[b, t, rs.randint(V)] = 1
        else:
            plan_np[b, t, rs.permutation(V)[:V // 2]] = 1
plan, allow = torch.from_numpy(plan_np).to(dev), allow.to(dev)
tokens = torch.empty(B, T, dtype=torch.int64, device=dev)
ws = torch.empty(lib.arvae_tick_free_run_ws_floats(H), dtype=torch.float32, device=dev)
p = lambda t: ctypes.c_void_p(t.data_ptr())
tw = _lib.TickWeights(*[p(t) for t in weights])
head = [ctypes.byref(tw), p(h0a), p(h0b), ctypes.c_int64(0), p(gib), p(ptab), None, ctypes.c_float(1.0)] + \
       [ctypes.c_int32(v) for v in (B, beats, tpb, H, V)]
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
flt = _lib.SampleFilter(args.top_k, args.top_p, p(allow))
cuts = _lib.SampleFilter(args.top_k, args.top_p, None)
npl = _lib.NotePlan(p(plan), T * V, V)
one = ctypes.c_float(1.0)
picks = {'argmax': lambda: lib.arvae_tick_free_run(*head, p(tokens), p(ws), stream),
         'filtered': lambda: lib.arvae_tick_free_run_filtered(*head, p(u), one, ctypes.byref(flt), p(tokens), p(ws), stream),
         'planned': lambda: lib.arvae_tick_free_run_planned(*head, p(u), one, ctypes.byref(cuts), ctypes.byref(npl), p(tokens), p(ws), stream)}
if other is not None:
    picks['argmax_other_lib'] = lambda: other.arvae_tick_free_run(*head, p(tokens), p(ws), stream)
    picks['filtered_other_lib'] = lambda: other.arvae_tick_free_run_filtered(*head, p(u), one, ctypes.byref(flt), p(tokens), p(ws), stream)


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


out = {'launches': args.launches, 'top_k': args.top_k, 'top_p': args.top_p, 'other_lib': args.other_lib}
for r in range(args.repeats):                                   # the picks alternate inside a repeat: drift hits all alike
    for name, launch in picks.items():
        out.setdefault(name + '_us', []).append(round(median_us(launch), 2))
for name in picks:
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
out['planned_over_filtered'] = round(out['planned_median_us'] / out['filtered_median_us'], 4)
assert picks['planned']() == 0                                  # (the last timed launch may have been another pick)
torch.cuda.synchronize()
assert int(tokens.min()) >= 0 and int(tokens.max()) < V and bool(plan.gather(2, tokens[..., None]).all())

# HierarchicalDecoder.generate with the same cuts: without a plan, with it in one launch, with it tick by tick
from arvae_amd.measure_vae import HierarchicalDecoder
torch.manual_seed(0)
dec = HierarchicalDecoder(10, V, 32, 2, H, 0.0).to(dev).eval()
z = rnd(B, 32, s=1.0)
configs = {'generate_filtered': ('0', dict(allowed=allow.cpu())), 'generate_planned_one_launch': ('0', dict(plan=plan_np)),
           'generate_planned_tick_by_tick': ('1', dict(plan=plan_np))}


def generate_us(mode, kw, calls):
    os.environ['ARVAE_TICK_STEPWISE'] = mode
    run = lambda: dec.generate(z, uniforms=u, temperature=1.0, top_k=args.top_k, top_p=args.top_p, **kw)
    for _ in range(3):
        run()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


for r in range(args.repeats):
    for name, (mode, kw) in configs.items():
        out.setdefault(name + '_us', []).append(round(generate_us(mode, kw, 5 if mode == '1' else 20), 1))
for name in configs:
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
print(json.dumps(out))

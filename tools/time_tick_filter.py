"""Time of the free-running tick decoder with filtered sampling (csrc/tick_decoder.hip, PICK_FILTERED: top-k, nucleus and note mask)
beside the unfiltered multinomial pass: B = 256, H = 128, 4 beats x 6 ticks, vocabulary 35, no dropout (generation).
  library level: one call = the two weight prep launches + the tick kernel, HIP events around every call, median over --launches calls
  after a warm-up, --repeats times, the picks alternating inside a repeat (tools/time_tick_pick.py's method);
  decoder level: HierarchicalDecoder._free_running_tokens with the same cuts, one launch against tick by tick (ARVAE_TICK_STEPWISE=1:
  per tick the dense launches, the gate launches and arvae_row_sample_filtered), host timer around a synchronised call.
--unfiltered-lib takes another build of the library (an earlier commit's) for the unfiltered pass: two builds are compared by
running this once each, alternately, on the same device.

    python tools/time_tick_filter.py [--unfiltered-lib path/to/libarvae_hip.so] [--launches 60] [--repeats 5]
"""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from arvae_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--unfiltered-lib', default=None)
ap.add_argument('--launches', type=int, default=60)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--top_k', type=int, default=4)
ap.add_argument('--top_p', type=float, default=0.9)
args = ap.parse_args()
lib = _lib.load()
other = ctypes.CDLL(args.unfiltered_lib) if args.unfiltered_lib else None
dev = torch.device('cuda:0')
B, H, V, beats, tpb = 256, 128, 35, 4, 6
g = torch.Generator(device='cpu').manual_seed(1)
def rnd(*shape, s=0.1): return (torch.randn(*shape, generator=g) * s).to(dev)
weights = (rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(V, H, s=0.5), rnd(V))
h0a, h0b = torch.tanh(rnd(beats * B, H, s=1.0)), torch.tanh(rnd(beats * B, H, s=1.0))
gib, ptab = rnd(beats * B, 3 * H, s=0.5), rnd(V + 1, 3 * H, s=0.5)
u = torch.rand(B, beats * tpb, generator=g).clamp_(min=2.0 ** -32).to(dev)
allow = torch.ones(V, dtype=torch.uint8)
allow[[1, 2, 4]] = 0                                            # START, END and None of the folk vocabulary
allow = allow.to(dev)
tokens = torch.empty(B, beats * tpb, dtype=torch.int64, device=dev)
ws = torch.empty(lib.arvae_tick_free_run_ws_floats(H), dtype=torch.float32, device=dev)
p = lambda t: ctypes.c_void_p(t.data_ptr())
tw = _lib.TickWeights(*[p(t) for t in weights])
head = [ctypes.byref(tw), p(h0a), p(h0b), ctypes.c_int64(0), p(gib), p(ptab), None, ctypes.c_float(1.0)] + \
       [ctypes.c_int32(v) for v in (B, beats, tpb, H, V)]
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
flt = _lib.SampleFilter(args.top_k, args.top_p, p(allow))
picks = {'multinomial': lambda: lib.arvae_tick_free_run_sampled(*head, p(u), ctypes.c_float(1.0), p(tokens), p(ws), stream),
         'filtered': lambda: lib.arvae_tick_free_run_filtered(*head, p(u), ctypes.c_float(1.0), ctypes.byref(flt), p(tokens), p(ws), stream)}
if other is not None:
    picks['multinomial_other_lib'] = lambda: other.arvae_tick_free_run_sampled(*head, p(u), ctypes.c_float(1.0), p(tokens), p(ws), stream)


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


out = {'launches': args.launches, 'top_k': args.top_k, 'top_p': args.top_p, 'unfiltered_lib': args.unfiltered_lib}
for r in range(args.repeats):                                   # the picks alternate inside a repeat: drift hits all alike
    for name, launch in picks.items():
        out.setdefault(name + '_us', []).append(round(median_us(launch), 2))
for name in picks:
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
out['filtered_over_multinomial'] = round(out['filtered_median_us'] / out['multinomial_median_us'], 4)
assert picks['filtered']() == 0                                 # (the last timed launch may have been an unfiltered one)
torch.cuda.synchronize()
assert int(tokens.min()) >= 0 and int(tokens.max()) < V and bool(allow[tokens].all())

# the decoder's feedback pass with the same cuts, one launch against tick by tick
from arvae_amd.measure_vae import HierarchicalDecoder
torch.manual_seed(0)
dec = HierarchicalDecoder(10, V, 32, 2, H, 0.0).to(dev).eval()
beat_out = torch.tanh(rnd(beats, B, H, s=1.0))
h0 = [h0a, h0b]
dec._filter = (args.top_k, args.top_p, allow)


def pass_us(mode, calls):
    os.environ['ARVAE_TICK_STEPWISE'] = mode
    with torch.no_grad():
        for _ in range(3):
            dec._free_running_tokens(beat_out, h0, gib[:, :H].contiguous(), None, u)
        times = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec._free_running_tokens(beat_out, h0, gib[:, :H].contiguous(), None, u)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


for r in range(args.repeats):
    out.setdefault('decoder_one_launch_us', []).append(round(pass_us('0', 20), 1))
    out.setdefault('decoder_tick_by_tick_us', []).append(round(pass_us('1', 5), 1))
for name in ('decoder_one_launch', 'decoder_tick_by_tick'):
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
print(json.dumps(out))

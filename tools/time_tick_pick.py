"""Time of one launch of the free-running tick decoder (csrc/tick_decoder.hip: the two weight prep launches + tick_free_run_h2_kernel), top-1 feedback and -- where the library
has it -- multinomial feedback: B = 256, H = 128, 4 beats x 6 ticks, vocabulary 35, dropout 0.5.  HIP events around every launch,
median over --launches launches after a warm-up, --repeats times (the spread of the medians is the yardstick for a difference).
--lib takes any build of the library (an earlier commit's too: the entry points are called through ctypes directly, whatever its ABI
number), so two builds are compared by running this once each, alternately, on the same device.

    python tools/time_tick_pick.py [--lib path/to/libarvae_hip.so] [--launches 60] [--repeats 5]
"""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from arvae_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--lib', default=_lib.LIB_PATH)
ap.add_argument('--launches', type=int, default=60)
ap.add_argument('--repeats', type=int, default=5)
args = ap.parse_args()
lib = ctypes.CDLL(args.lib)
dev = torch.device('cuda:0')
B, H, V, beats, tpb = 256, 128, 35, 4, 6
g = torch.Generator(device='cpu').manual_seed(1)
def rnd(*shape, s=0.1): return (torch.randn(*shape, generator=g) * s).to(dev)
weights = (rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(V, H, s=0.5), rnd(V))
h0a, h0b = torch.tanh(rnd(beats * B, H, s=1.0)), torch.tanh(rnd(beats * B, H, s=1.0))
gib, ptab = rnd(beats * B, 3 * H, s=0.5), rnd(V + 1, 3 * H, s=0.5)
mask = (torch.rand(beats * tpb, B, H, generator=g) >= 0.5).to(torch.uint8).to(dev)
u = torch.rand(B, beats * tpb, generator=g).clamp_(min=2.0 ** -32).to(dev)
tokens = torch.empty(B, beats * tpb, dtype=torch.int64, device=dev)
lib.arvae_tick_free_run_ws_floats.restype = ctypes.c_int64
ws = torch.empty(lib.arvae_tick_free_run_ws_floats(ctypes.c_int32(H)), dtype=torch.float32, device=dev)
p = lambda t: ctypes.c_void_p(t.data_ptr())
tw = _lib.TickWeights(*[p(t) for t in weights])
head = [ctypes.byref(tw), p(h0a), p(h0b), ctypes.c_int64(0), p(gib), p(ptab), p(mask), ctypes.c_float(2.0)] + \
       [ctypes.c_int32(v) for v in (B, beats, tpb, H, V)]
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
picks = {'argmax': lambda: lib.arvae_tick_free_run(*head, p(tokens), p(ws), stream)}
if hasattr(lib, 'arvae_tick_free_run_sampled'):
    picks['multinomial'] = lambda: lib.arvae_tick_free_run_sampled(*head, p(u), ctypes.c_float(1.0), p(tokens), p(ws), stream)


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


out = {'lib': args.lib, 'launches': args.launches}
for r in range(args.repeats):                                   # the picks alternate inside a repeat: drift hits both alike
    for name, launch in picks.items():
        out.setdefault(name + '_us', []).append(round(median_us(launch), 2))
for name in picks:
    out[name + '_median_us'] = statistics.median(out[name + '_us'])
if 'multinomial' in picks:
    out['multinomial_over_argmax'] = round(out['multinomial_median_us'] / out['argmax_median_us'], 4)
    assert int(tokens.min()) >= 0 and int(tokens.max()) < V
print(json.dumps(out))

"""Time of the beam search of the tick decoder (csrc/beam_decoder.hip) at B = 256, H = 128, 4 beats x 6 ticks, vocabulary 35, widths
W = 2, 4, 8, 16, beside its floor and its tick-by-tick path:
  library level: one call = the two weight prep launches + the kernel.  `beam`: arvae_tick_beam_search; `floor`: the existing argmax
  free run (arvae_tick_free_run) over the same B * W rows -- the same recurrences with no selection and no permutation;
  decoder level: HierarchicalDecoder._beam_history, one launch against tick by tick (ARVAE_TICK_STEPWISE=1: per tick the dense
  launches, the gate launches, arvae_beam_select and the states' gather), the input projections' launches included in both.
HIP events around every call, the stream synchronised between calls, median over --launches calls after a warm-up, --repeats times, the
variants alternating inside a repeat (tools/time_tick_filter.py's method).

    python tools/time_tick_beam.py [--launches 40] [--repeats 3] [--widths 2,4,8,16]
"""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from arvae_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--launches', type=int, default=40)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--widths', default='2,4,8,16')
args = ap.parse_args()
lib = _lib.load()
dev = torch.device('cuda:0')
B, H, V, beats, tpb = 256, 128, 35, 4, 6
T = beats * tpb
g = torch.Generator(device='cpu').manual_seed(1)
def rnd(*shape, s=0.1): return (torch.randn(*shape, generator=g) * s).to(dev)
weights = (rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(V, H, s=0.5), rnd(V))
h0a, h0b = torch.tanh(rnd(beats * B, H, s=1.0)), torch.tanh(rnd(beats * B, H, s=1.0))
gib, ptab = rnd(beats * B, 3 * H, s=0.5), rnd(V + 1, 3 * H, s=0.5)
p = lambda t: ctypes.c_void_p(t.data_ptr())
tw = _lib.TickWeights(*[p(t) for t in weights])
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
ws = torch.empty(lib.arvae_tick_beam_search_ws_floats(H), dtype=torch.float32, device=dev)
i32 = ctypes.c_int32

from arvae_amd.measure_vae import HierarchicalDecoder
torch.manual_seed(0)
dec = HierarchicalDecoder(10, V, 32, 2, H, 0.0).to(dev).eval()
beat_out = torch.tanh(rnd(beats, B, H, s=1.0))


def median_us(launch, calls, warm=5):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


out = {'launches': args.launches, 'repeats': args.repeats, 'batch': B, 'hidden': H, 'vocab': V}
for W in [int(w) for w in args.widths.split(',')]:
    parents = torch.empty(B, T, W, dtype=torch.int32, device=dev)
    tokens = torch.empty(B, T, W, dtype=torch.int64, device=dev)
    hist = torch.empty(B, T, W, dtype=torch.float32, device=dev)
    seqs = torch.empty(B, W, T, dtype=torch.int64, device=dev)
    scores = torch.empty(B, W, dtype=torch.float32, device=dev)
    # the floor's inputs: every code's rows W times (row = beat * B * W + code * W + k)
    wide = lambda t: t.view(beats, B, -1).repeat_interleave(W, 1).reshape(beats * B * W, -1).contiguous()
    h0aw, h0bw, gibw = wide(h0a), wide(h0b), wide(gib)
    free = torch.empty(B * W, T, dtype=torch.int64, device=dev)

    def beam():
        assert lib.arvae_tick_beam_search(ctypes.byref(tw), p(h0a), p(h0b), ctypes.c_int64(0), p(gib), p(ptab), i32(B), i32(beats), i32(tpb),
                                          i32(H), i32(V), i32(W), None, i32(V), p(parents), p(tokens), p(hist), p(seqs), p(scores), p(ws),
                                          stream) == 0

    def floor():
        assert lib.arvae_tick_free_run(ctypes.byref(tw), p(h0aw), p(h0bw), ctypes.c_int64(0), p(gibw), p(ptab), None, ctypes.c_float(1.0),
                                       i32(B * W), i32(beats), i32(tpb), i32(H), i32(V), p(free), p(ws), stream) == 0

    def decoder(mode):
        def run():
            os.environ['ARVAE_TICK_STEPWISE'] = mode
            with torch.no_grad():
                dec._beam_history(beat_out, W, None, V)
        return run

    variants = {'beam': (beam, args.launches), 'floor': (floor, args.launches), 'decoder_one_launch': (decoder('0'), args.launches),
                'decoder_tick_by_tick': (decoder('1'), max(3, args.launches // 8))}
    res = {}
    for r in range(args.repeats):                               # the variants alternate inside a repeat: drift hits all alike
        for name, (launch, calls) in variants.items():
            res.setdefault(name + '_us', []).append(round(median_us(launch, calls), 1))
    for name in variants:
        res[name + '_median_us'] = statistics.median(res[name + '_us'])
    res['beam_over_floor'] = round(res['beam_median_us'] / res['floor_median_us'], 3)
    res['tick_by_tick_over_one_launch'] = round(res['decoder_tick_by_tick_median_us'] / res['decoder_one_launch_median_us'], 2)
    # width 1 of the floor's rows is what the beam's first hypothesis starts as: sanity of the histories
    beam()
    torch.cuda.synchronize()
    assert int(tokens.min()) >= 0 and int(tokens.max()) < V and bool(torch.isfinite(scores).all())
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    out[f'width_{W}'] = res
    os.environ['ARVAE_TICK_STEPWISE'] = '0'
print(json.dumps(out))

"""Time of one create_latent_gifs render (ops.render_frames, csrc/render.hip) beside the path it replaces, on logits of the
figure's own shape: Morpho-MNIST 6 attributes x 10 points of 28 x 28 -> 10 frames of 32 x 182 x 3; dSprites 5 x 10 of 64 x 64 ->
10 frames of 68 x 332 x 3.
  render: the launch alone between HIP events, and launch + the copy of the uint8 frames to the host on a host clock;
  before: torch.sigmoid on the device, the float images copied to the host, logging_utils.image_grid per frame (the Python cell
  loop), .mul(255).clamp(0, 255).byte().permute(1, 2, 0): host clock around the whole, which starts and ends synchronised.
Median over --calls calls after a warm-up, --repeats times, the two alternating inside a repeat.

    python tools/time_figures.py [--calls 50] [--repeats 5]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from arvae_amd import ops
from arvae_amd.logging_utils import image_grid

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=50)
ap.add_argument('--repeats', type=int, default=5)
args = ap.parse_args()
dev = torch.device('cuda:0')
P = 10


def render_event_us(logits, cells):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    cells_dev = torch.from_numpy(cells.astype(np.int32)).to(dev)
    n, h, w = logits.shape
    hg, wg = ops.render_geometry(h, w, cells.shape[1], 8, 2)
    out = torch.empty(cells.shape[0], hg, wg, 3, dtype=torch.uint8, device=dev)
    lib = ops._lib.load()
    call = lambda: lib.arvae_render_frames(ops._ptr(logits), n, h, w, ops._ptr(cells_dev), cells.shape[0], cells.shape[1], 8, 2, 1.0,
                                           ops.RENDER_SRC_LOGITS | ops.RENDER_RGB, ops._ptr(out), ops._stream())
    for _ in range(10):
        assert call() == 0
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        assert call() == 0
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def host_us(fn):
    for _ in range(5):
        fn()
    times = []
    for _ in range(args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


out = {'calls': args.calls, 'repeats': args.repeats}
for kind, hw, attrs in (('mnist', 28, 6), ('dsprites', 64, 5)):
    g = torch.Generator().manual_seed(0)
    logits = (3.0 * torch.randn(attrs * P, hw, hw, generator=g)).to(dev)
    cells = np.arange(attrs * P).reshape(attrs, P).T

    def new():
        return ops.render_frames(logits, cells).cpu().numpy()

    def before():
        probs = torch.sigmoid(logits).view(attrs, P, 1, hw, hw).transpose(0, 1).cpu()
        return [image_grid(probs[n], attrs).mul(255).clamp(0, 255).byte().expand(3, -1, -1).permute(1, 2, 0).numpy() for n in range(P)]

    a, b = new(), np.stack([np.ascontiguousarray(f) for f in before()])
    assert a.shape == b.shape and int(np.abs(a.astype(int) - b.astype(int)).max()) <= 1      # (the sigmoids may differ in the last bit)
    for r in range(args.repeats):
        out.setdefault(f'{kind}_render_launch_us', []).append(round(render_event_us(logits, cells), 2))
        out.setdefault(f'{kind}_render_to_host_us', []).append(round(host_us(new), 1))
        out.setdefault(f'{kind}_before_to_host_us', []).append(round(host_us(before), 1))
    out[f'{kind}_differing_bytes'] = int((a != b).sum())
for key in [k for k in out if k.endswith('_us')]:
    out[key + '_median'] = statistics.median(out[key])
    out[key + '_spread'] = round(max(out[key]) - min(out[key]), 2)
print(json.dumps(out))

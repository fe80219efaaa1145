"""Time of the scatter figures (ops.render_scatter, csrc/scatter.hip) and of MeasureVAETrainer.plot_latent_surface at the command
line's size: 200 x 200 = 40 000 codes over the plane, four attributes, figures of 485 x 360.  The model has the command line's
default sizes (hidden 128, 32 latent dimensions) and random weights on the synthetic vocabulary: the times do not depend on them.
  render: the launch alone between HIP events, for one figure and for four (the points are the grid's, the values its labels);
  surface: the whole plot_latent_surface call for four attributes on a host clock, and its parts -- decode and labels
  (compute_latent_surface), the render launch, the frames' copy to the host, the four PNG files -- each on a host clock of its own;
  baseline: the same surface decoded in minibatches of 500 codes (compute_latent_surface(chunk=500)), once for all attributes and
  once per attribute as the reference's plot_latent_surface does it.
Median over --calls calls after a warm-up, --repeats times.

    python tools/time_scatter.py [--calls 20] [--repeats 3]
"""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch
from arvae_amd import figures, ops, synthetic as syn
from arvae_amd.measure_vae import MeasureVAE
from arvae_amd.measure_vae_trainer import MeasureVAETrainer

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=20)
ap.add_argument('--repeats', type=int, default=3)
args = ap.parse_args()
dev = torch.device('cuda:0')
ATTRS = ['rhy_complexity', 'pitch_range', 'note_density', 'contour']


class Folk:
    class_name = '4by4_FolkNBarDataset_1_'
    n_bars = 1

    def __init__(self):
        self.index2note_dicts, self.note2index_dicts = syn.measure_vocabulary()

    def __repr__(self):
        return self.class_name


os.environ['ARVAE_MODEL_DIR'] = tempfile.mkdtemp()
torch.manual_seed(0)
dataset = Folk()
model = MeasureVAE(dataset, 10, 2, 2, 128, 0.5, 32, 2, 128, 0.5, False, 'folk')
trainer = MeasureVAETrainer(dataset, model, reg_type=('all',), reg_dim=(0, 1, 2, 3))
trainer.cuda()
model.eval()
base = torch.randn(32)
grid, labels = trainer.compute_latent_surface(0, 1, 0.05, base)
n = grid.shape[0] * grid.shape[1]
points4 = grid.reshape(1, n, 2).expand(4, n, 2).contiguous()
values4 = labels.reshape(n, 4).t().contiguous()
vlo, vhi = values4.amin(1).cpu().tolist(), values4.amax(1).cpu().tolist()


def launch_event_us(f):
    out = torch.empty(f, 360, 485, 3, dtype=torch.uint8, device=dev)
    call = lambda: ops.render_scatter(points4[:f], values4[:f], (-5.0, 5.0), (-5.0, 5.0), vlo[:f], vhi[:f], out=out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def host_us(fn, calls):
    fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


frames4 = ops.render_scatter(points4, values4, (-5.0, 5.0), (-5.0, 5.0))
host_frames = frames4.cpu().numpy()
folder = tempfile.mkdtemp()
few = max(3, args.calls // 5)
out = {'calls': args.calls, 'repeats': args.repeats, 'points': n, 'frame_bytes': int(frames4[0].numel())}
for r in range(args.repeats):
    out.setdefault('render_launch_1_us', []).append(round(launch_event_us(1), 2))
    out.setdefault('render_launch_4_us', []).append(round(launch_event_us(4), 2))
    out.setdefault('plot_latent_surface_4_us', []).append(round(host_us(lambda: trainer.plot_latent_surface(ATTRS, 0, 1, 0.05, base), few), 1))
    out.setdefault('decode_and_labels_us', []).append(round(host_us(lambda: trainer.compute_latent_surface(0, 1, 0.05, base), few), 1))
    out.setdefault('render_4_found_bounds_us', []).append(round(host_us(lambda: ops.render_scatter(points4, values4, (-5.0, 5.0), (-5.0, 5.0)), args.calls), 1))
    out.setdefault('copy_4_frames_us', []).append(round(host_us(lambda: frames4.cpu(), args.calls), 1))
    out.setdefault('png_4_files_us', []).append(round(host_us(lambda: [figures.write_png(host_frames[i], os.path.join(folder, f'{i}.png')) for i in range(4)], few), 1))
    out.setdefault('decode_chunks_of_500_us', []).append(round(host_us(lambda: trainer.compute_latent_surface(0, 1, 0.05, base, chunk=500), few), 1))
    out.setdefault('decode_chunks_of_500_per_attribute_us', []).append(round(host_us(
        lambda: [trainer.compute_latent_surface(0, 1, 0.05, base, [a], chunk=500) for a in ATTRS], few), 1))
for key in [k for k in out if k.endswith('_us')]:
    out[key + '_median'] = statistics.median(out[key])
    out[key + '_spread'] = round(max(out[key]) - min(out[key]), 2)
print(json.dumps(out))

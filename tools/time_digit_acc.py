#!/usr/bin/env python3
"""Throughput of the digit classifier (arvae_amd.mnist_resnet, csrc/resnet18.hip) at the two batch sizes the evaluation issues:
128 (inputs, reconstructions) and 1280 (a latent sweep: 10 points x 128 codes).

One JSON line per measurement:
  hip         the one-call forward: median of --reps timed calls (HIP events) after --warmup calls; images/s; the network's
              algorithmic FLOP/s (66.0 MFLOP per image, every tap counted) and its share of the three-term bf16 roof (the bf16
              MFMA peak / 6 partial products); the live-tap FLOP/s (what the kernels multiply) beside it
  hip_split   the per-launch split: the same network through the per-layer entry points under ops.profile_begin / profile_end
              (HIP events around each launch), median over --reps passes
  torch_gpu   yardstick: the float32 torch.nn restatement (tests/resnet_ref.py) on the same GPU, same event timing
  torch_cpu   yardstick: the same restatement on the host (torch.get_num_threads() threads), wall clock, median of 3
  end_to_end  seconds of ImageVAETrainer.get_resnet_accuracy on a synthetic t10k-sized split (--images, batch 128), random VAE

    python tools/time_digit_acc.py [--reps 20] [--warmup 5] [--images 10000] [--no-cpu] [--no-end-to-end]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import arvae_amd  # noqa: E402,F401
import resnet_ref  # noqa: E402
from arvae_amd import ops  # noqa: E402
from arvae_amd.mnist_resnet import MnistResNet  # noqa: E402

PEAK_BF16_MFMA_TFLOPS = 2500.0                   # MI355X dense bf16 MFMA (bench.py's figure)
X3_PRODUCTS = 6                                  # partial products per MAC of the three-term split


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return times


def live_flop_per_image(model):
    flop = 2.0 * 196 * 64 * 49 + 2.0 * 512 * 10
    for g, _, _, _ in model.conv_sequence():
        flop += 2.0 * g.hout * g.hout * g.cout * g.cin * len(ops.resnet18_live_taps(g))
    return flop


def rate_row(kind, batch, times, flop_per_image, **extra):
    med = statistics.median(times)
    row = {'kind': kind, 'batch': batch, 'calls': len(times), 'median_ms': round(med * 1e3, 4), 'min_ms': round(min(times) * 1e3, 4),
           'max_ms': round(max(times) * 1e3, 4), 'images_per_s': round(batch / med, 1),
           'algorithmic_tflops': round(batch * flop_per_image / med / 1e12, 3)}
    row.update(extra)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--images', type=int, default=10000)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--no-end-to-end', action='store_true')
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps: at least 20 timed calls')
    if not torch.cuda.is_available():
        raise SystemExit('time_digit_acc.py needs a GPU: nothing here can be timed on the CPU')
    dev = torch.device('cuda:0')
    sd = resnet_ref.random_state_dict(7)
    model = MnistResNet()
    model.load_state_dict(sd)
    model.to(dev).eval()
    ref_gpu = resnet_ref.build(sd, torch.float32).to(dev)
    ref_cpu = resnet_ref.build(sd, torch.float32)
    flop, live = ops.RESNET18_FLOP_PER_IMAGE, live_flop_per_image(model)
    roof = PEAK_BF16_MFMA_TFLOPS / X3_PRODUCTS
    for batch in (128, 1280):
        x_host = torch.from_numpy(resnet_ref.stroke_images(batch, batch))
        x = x_host.to(dev)
        model.classify(x)                                            # (prepares the weights)
        times = event_times(lambda: model.classify(x), args.reps, args.warmup)
        med = statistics.median(times)
        print(json.dumps(rate_row('hip', batch, times, flop, live_tap_tflops=round(batch * live / med / 1e12, 3),
                                  roof_tflops_fp32_equivalent=round(roof, 1),
                                  algorithmic_share_of_roof=round(batch * flop / med / 1e12 / roof, 5),
                                  live_tap_share_of_roof=round(batch * live / med / 1e12 / roof, 5))), flush=True)
        # per-launch split (a separate pass: the events slow the host)
        passes = []
        for _ in range(args.warmup + args.reps):
            ops.profile_begin()
            model.forward_layerwise(x)
            passes.append(ops.profile_end())
        passes = passes[args.warmup:]
        split = {}
        for name in passes[0]:
            ms = statistics.median(p[name]['ms'] for p in passes)
            split[name] = {'launches': passes[0][name]['calls'], 'median_ms': round(ms, 4),
                           'tflops': round(passes[0][name]['flop'] / (ms * 1e-3) / 1e12, 3) if ms > 0 else None}
        total = sum(v['median_ms'] for v in split.values())
        print(json.dumps({'kind': 'hip_split', 'batch': batch, 'sum_ms': round(total, 4), 'launches': split}), flush=True)
        with torch.no_grad():
            times = event_times(lambda: torch.softmax(ref_gpu(x), 1).argmax(1), args.reps, args.warmup)
            print(json.dumps(rate_row('torch_gpu', batch, times, flop)), flush=True)
            if not args.no_cpu:
                ref_cpu(x_host)
                cpu = []
                for _ in range(3):
                    t = time.perf_counter()
                    torch.softmax(ref_cpu(x_host), 1).argmax(1)
                    cpu.append(time.perf_counter() - t)
                print(json.dumps(rate_row('torch_cpu', batch, cpu, flop, threads=torch.get_num_threads())), flush=True)
    if not args.no_end_to_end:
        print(json.dumps(end_to_end(model, dev, args.images)), flush=True)


def end_to_end(resnet, dev, n):
    """get_resnet_accuracy over n synthetic Morpho-MNIST images held on the device, batch 128, randomly initialised MnistVAE"""
    from arvae_amd import synthetic as syn
    from arvae_amd.data.loaders import DeviceLoader
    from arvae_amd.image_vae import MnistVAE
    from arvae_amd.image_vae_trainer import ImageVAETrainer

    class MorphoMnistDataset:
        def __init__(self):
            x, lab = syn.mnist_batch(n, seed=3)
            imgs = torch.from_numpy(np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)).to(dev)
            self.split = (imgs, torch.from_numpy((np.arange(n) % 10).astype(np.int64)).to(dev), torch.from_numpy(lab.astype(np.float32)).to(dev))

        def data_loaders(self, batch_size, split=(0.85, 0.10), shard=None):
            return tuple(DeviceLoader(self.split, 0, n, batch_size, shuffle=False, u8_scale=1.0 / 255.0, shard=shard) for _ in range(3))
    torch.manual_seed(0)
    trainer = ImageVAETrainer(MorphoMnistDataset(), MnistVAE(), rand=0)
    trainer.cuda()
    trainer.metrics = {'interpretability': {'area': (1, 0.0), 'length': (2, 0.0), 'thickness': (3, 0.0), 'slant': (4, 0.0), 'width': (5, 0.0),
                                            'height': (6, 0.0), 'mean': (-1, 0.0)}}
    trainer.get_resnet_accuracy(batch_size=128, resnet_model=resnet)          # warm-up pass
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = trainer.get_resnet_accuracy(batch_size=128, resnet_model=resnet)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return {'kind': 'end_to_end', 'images': n, 'batch': 128, 'classified_images': n * 72, 'median_s': round(statistics.median(times), 3),
            'min_s': round(min(times), 3), 'max_s': round(max(times), 3), 'digit_pred_acc': out['digit_pred_acc']}


if __name__ == '__main__':
    main()

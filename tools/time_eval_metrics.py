#!/usr/bin/env python3
"""Wall time of the disentanglement-metric suite (arvae_amd.evaluation.compute_disentanglement_metrics) on the three workload
shapes (arvae_amd.synthetic.EVAL_SHAPES: dsprites 25,728 x 10 / 5 attributes, mnist 25,728 x 16 / 6, measure 51,456 x 32 / 4).

For each shape, one JSON line: the suite's wall time (median of --reps after a warm-up run), split into host preprocessing
(sklearn's scaling + noise draws, arvae_amd.evaluation.prepare_inputs) and the rest, plus the summed device time of the KSG
launches (HIP events around each call).  When scikit-learn is importable (and not --no-sklearn), also the CPU time of the
reference's suite: the same KSG calls through sklearn.feature_selection.mutual_info_regression (3 * A calls over all codes +
A entropies; the reference's moment / rank work is not included, it is small next to them).

    python tools/time_eval_metrics.py [--reps 3] [--kinds dsprites,mnist,measure] [--no-sklearn] [--no-device]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import arvae_amd  # noqa: E402,F401
from arvae_amd import evaluation as ev  # noqa: E402
from arvae_amd import synthetic as syn  # noqa: E402


def time_device(codes, attrs, names, reps):
    import torch
    host = []
    events = []
    prepare, ksg = ev.prepare_inputs, ev.ksg_mi

    def timed_prepare(*a, **kw):
        t = time.perf_counter()
        out = prepare(*a, **kw)
        host.append(time.perf_counter() - t)
        return out

    def timed_ksg(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ksg(*a, **kw)
        e1.record()
        events.append((e0, e1))
        return out
    ev.prepare_inputs, ev.ksg_mi = timed_prepare, timed_ksg
    try:
        rows = []
        for r in range(reps + 1):
            host.clear()
            events.clear()
            torch.cuda.synchronize()
            t = time.perf_counter()
            ev.compute_disentanglement_metrics(codes, attrs, names, random_state=r)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
            rows.append((wall, sum(host), sum(a.elapsed_time(b) for a, b in events) / 1e3, len(events)))
    finally:
        ev.prepare_inputs, ev.ksg_mi = prepare, ksg
    rows = sorted(rows[1:])
    return rows[len(rows) // 2]


def time_sklearn(codes, attrs):
    from sklearn.feature_selection import mutual_info_regression
    t = time.perf_counter()
    a = attrs.shape[1]
    for c in range(3 * a):
        mutual_info_regression(codes, attrs[:, c % a], random_state=c)
    for j in range(a):
        mutual_info_regression(attrs[:, j:j + 1], attrs[:, j], random_state=3 * a + j)
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kinds', default='dsprites,mnist,measure')
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--no-device', action='store_true')
    args = ap.parse_args()
    have_sklearn = False
    if not args.no_sklearn:
        try:
            import sklearn  # noqa: F401
            have_sklearn = True
        except ImportError:
            pass
    for kind in args.kinds.split(','):
        codes, attrs, names = syn.eval_metric_inputs(kind, 0)
        row = {'kind': kind, 'n': int(codes.shape[0]), 'codes': int(codes.shape[1]), 'attributes': int(attrs.shape[1]),
               'ksg_columns': int(3 * codes.shape[1] * attrs.shape[1] + attrs.shape[1])}
        if not args.no_device:
            wall, host, device, calls = time_device(codes, attrs, names, args.reps)
            row.update(suite_s=round(wall, 4), host_prep_s=round(host, 4), other_s=round(wall - host, 4),
                       ksg_device_s=round(device, 4), ksg_calls=calls)
        if have_sklearn:
            row['sklearn_cpu_s'] = round(time_sklearn(codes, attrs), 2)
            if 'suite_s' in row:
                row['speedup'] = round(row['sklearn_cpu_s'] / row['suite_s'], 1)
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""tools/stamp.py <family> [args]: run a kernel family's workload on a phase-stamped build and print its phase timeline.

The instrument is ar-vae_amd/csrc/stamps.h: one -DARVAE_STAMPS_<FAMILY> flag per family, armed one at a time.  Build the
stamped library beside the product one and name it in ARVAE_LIB (else the product library is loaded, which carries no stamps):

    bash tools/build_diag.sh lib_stamps_mid midblock.hip -DARVAE_STAMPS_MID
    ARVAE_LIB=$PWD/tools/bin/lib_stamps_mid.so python tools/stamp.py mid

FAMILIES below is the one list of the families: source file, flag, table shape (tests/test_stamp_builds.py holds it to the
declarations in csrc), phase names, the driver (the workload that launches the kernel) and the report.  This module imports
without torch or a GPU; the drivers import what they need.

    conv32 [n]            the <16> conv32 kernels: down32, up32, wgrad32 (n images, default 512)
    conv32 up32p [bwd]    the forward up32p launch of a fused dSprites step (bwd: the gated data gradient of conv2)
    d32k                  the LAST down32p launch of a dSprites forward pass
    wgr [lo] [n]          wgrad32r_kernel<lo> (default 16, 512 images)
    c64s [n]              one conv64s launch (64 -> 64 channels, 25x25 -> 22x22: the Morpho-MNIST layer; default 1024)
    midc, mid, dw         the clustered latent block / mid_forward_kernel / the dense weight-gradient tiles, dSprites B = 512
    rg                    a rows-GEMM weight gradient (6144 rows, 128 -> 384: the MeasureVAE's W_ih) and the same layer's forward
    s8                    a tile of conv_s8_h2_kernel, the last launch of a Morpho-MNIST training step
    gru [bwd]             a step of the GRU sequence kernels, T = 24, R = 256, H = 128 (-DGRU_STAMP_WAVE=w picks the wave)
    tick                  a tick of the free-running decoder, B = 256, H = 128, 4 beats x 6 ticks, vocabulary 35, dropout 0.5
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_LIB = os.path.join(ROOT, 'ar-vae_amd', 'libarvae_hip.so')


def reader(family):
    """read() -> the family's table as an int64 array of its `view` shape, through the library's arvae_debug_<family>_stamps"""
    import numpy as np
    import torch  # noqa: F401  (first: its HIP runtime has to be the process's only one, ar-vae_amd/_lib.py)
    f = FAMILIES[family]
    path = os.environ.get('ARVAE_LIB') or PRODUCT_LIB
    try:
        fn = getattr(ctypes.CDLL(path), f'arvae_debug_{family}_stamps')
    except AttributeError:
        name = f'lib_stamps_{family}'
        sys.exit(f'{path} has no {family} stamps (it was not built with -D{f["flag"]}).  Build and select a library that has:\n'
                 f'    bash tools/build_diag.sh {name} {f["source"]} -D{f["flag"]}\n'
                 f'    ARVAE_LIB=$PWD/tools/bin/{name}.so python tools/stamp.py {family}')
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    rows, slots, words = f['shape']
    count = rows * slots * words

    def read():
        buf = (ctypes.c_ulonglong * count)()
        rc = fn(buf, count)
        if rc != 0:
            sys.exit(f'arvae_debug_{family}_stamps returned {rc}')
        return np.array(buf, dtype=np.uint64).reshape(f.get('view', (rows, slots))).astype(np.int64)
    return read


def mean_max(names, d):
    """per phase the mean / max over the stamping workgroups; d[workgroup][phase] in wall-clock ticks (100 MHz)"""
    width = max(len(n) for n in names) + 2
    for n, m, mx in zip(names, d.mean(0) / 100.0, d.max(0) / 100.0):
        print(f'{n:{width}s} mean {m:6.2f} us   max {mx:6.2f} us')


def cycle_shares(names, sums, unit, note=''):
    """cycles per phase and share; sums = the phase sums and, last, the count of units (steps, ticks, tiles) they were summed over"""
    count, tot = int(sums[len(names)]), int(sum(sums[:len(names)]))
    width = max(len(n) for n in names) + 2
    for n, v in zip(names, sums):
        print(f'{n:{width}s} {v / count:8.0f} cycles/{unit} {100 * v / tot:5.1f}%')
    print(f'total {tot / count:.0f} cycles/{unit}{note}')


# The drivers: each runs its workload and yields once per table to read; what it yields goes to the family's report with the table.
def _torch():
    sys.path.insert(0, ROOT)
    import torch
    return torch, torch.device('cuda:0')


def _dsprites_steps(backward=True, step=True):
    """five dSprites training steps at B = 512 (bench.py's trainer): forward only, forward + backward, or whole steps"""
    torch, dev = _torch()
    import bench
    from arvae_amd import synthetic as syn
    trainer, _ = bench.build_trainer(dev, False)
    x, lab = syn.dsprites_batch(512, seed=1)
    x, lab = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    for i in range(5):
        trainer.zero_grad()
        loss, _ = trainer.loss_and_acc_for_batch((x, lab), 0, i, True)
        if backward:
            loss.backward()
        if step:
            trainer.step()
    torch.cuda.synchronize()


def _launch3(torch, launch):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()


def drive_conv32(args):
    if args[:1] == ['up32p']:
        backward = args[1:2] == ['bwd']              # then the last up32p launch is the gated data gradient of conv2
        _dsprites_steps(backward=backward, step=False)
        print('last up32p launch:', 'backward (EP_GATE_B)' if backward else 'forward (EP_RELU)')
        yield 'up32p'
        return
    torch, dev = _torch()
    from arvae_amd import ops
    n = int(args[0]) if args else 512
    link = ops.Link(32, 32, 32, 16, 16, 32, 4, 4, 2, 1)
    hi = torch.randn(n, 32, 32, 32, device=dev)
    lo = torch.randn(n, 16, 16, 32, device=dev)
    w = torch.randn(32, 32, 4, 4, device=dev) * 0.1
    b = torch.zeros(32, device=dev)
    g_lo = torch.randn(n, 16, 16, 32, device=dev)
    dw, db = torch.zeros_like(w), torch.zeros_like(b)
    for tag, launch in (('down32<16>', lambda: ops.link_down(link, n, ops._operand(hi), w, b, 1, None)),
                        ('up32<16>', lambda: ops.link_up(link, n, ops._operand(lo), w, b, 1, None)),
                        ('wgrad32<16>', lambda: ops.link_wgrad(link, n, ops._operand(g_lo), ops._operand(hi), dw, db, 1))):
        _launch3(torch, launch)
        yield tag, n


def drive_wgr(args):
    torch, dev = _torch()
    from arvae_amd import ops
    lo_sz = int(args[0]) if args else 16
    n = int(args[1]) if len(args) > 1 else 512
    link = ops.Link(2 * lo_sz, 2 * lo_sz, 32, lo_sz, lo_sz, 32, 4, 4, 2, 1)
    hi = torch.randn(n, 2 * lo_sz, 2 * lo_sz, 32, device=dev)
    lo = torch.randn(n, lo_sz, lo_sz, 32, device=dev)
    dw, db = torch.zeros(32, 32, 4, 4, device=dev), torch.zeros(32, device=dev)
    for _ in range(20):
        ops.link_wgrad(link, n, ops._operand(lo), ops._operand(hi), dw, db, 1)
    torch.cuda.synchronize()
    yield lo_sz, n


def drive_c64s(args):
    torch, dev = _torch()
    from arvae_amd import ops
    n = int(args[0]) if args else 1024
    link = ops.Link(25, 25, 64, 22, 22, 64, 4, 4, 1, 0)
    hi = torch.randn(n, 25, 25, 64, device=dev)
    w = torch.randn(64, 64, 4, 4, device=dev) * 0.05
    b = torch.zeros(64, device=dev)
    _launch3(torch, lambda: ops.link_down(link, n, ops._operand(hi), w, b, 2, None))
    yield


def drive_dsprites(args, **how):
    _dsprites_steps(**how)
    yield


def drive_rg(args):
    torch, dev = _torch()
    from arvae_amd import ops
    rows, n_in, n_out = 6144, 128, 384
    link = ops.Link.dense(n_in, n_out)
    x = torch.randn(rows, n_in, device=dev)
    g = torch.randn(rows, n_out, device=dev)
    w = torch.randn(n_out, n_in, device=dev) * 0.05
    b = torch.zeros(n_out, device=dev)
    dw, db = torch.zeros_like(w), torch.zeros_like(b)
    for tag, launch in (('weight gradient (K x rows operands, 128-row slices)',
                         lambda: ops.link_wgrad(link, rows, ops._operand(g), ops._operand(x), dw, db, 1)),
                        ('forward (rows x K operands, K = 128)', lambda: ops.link_down(link, rows, ops._operand(x), w, b, 0, None))):
        _launch3(torch, launch)
        yield tag, 4


def drive_s8(args):
    torch, dev = _torch()
    import bench
    step, eager, unit, _ = bench.build_side_workload('mnist', dev, 1024, 0, False, False)
    for i in range(3):
        eager(i)
    torch.cuda.synchronize()
    yield


def drive_gru(args):
    torch, dev = _torch()
    from arvae_amd import ops
    backward = args[:1] == ['bwd']
    T, R, H = 24, 256, 128
    gi = [torch.randn(T, R, 3 * H, device=dev).requires_grad_(backward) for _ in range(2)]
    w = [(torch.randn(3 * H, H, device=dev) * 0.05).requires_grad_(backward) for _ in range(2)]
    b = [torch.zeros(3 * H, device=dev).requires_grad_(backward) for _ in range(2)]
    gy = torch.randn(T, R, 2 * H, device=dev)
    for _ in range(3):
        with torch.set_grad_enabled(backward):
            y, _ = ops.gru_sequence(T, [(gi[0], w[0], b[0], None, False), (gi[1], w[1], b[1], None, True)])
        if backward:
            (y * gy).sum().backward()
    torch.cuda.synchronize()
    yield backward


def drive_tick(args):
    torch, dev = _torch()
    from arvae_amd import ops
    B, H, V, beats, tpb = 256, 128, 35, 4, 6
    g = torch.Generator(device='cpu').manual_seed(1)

    def rnd(*shape, s=0.1):
        return (torch.randn(*shape, generator=g) * s).to(dev)
    weights = (rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(3 * H, H), rnd(3 * H), rnd(V, H, s=0.5), rnd(V))
    h0a, h0b = torch.tanh(rnd(beats * B, H, s=1.0)), torch.tanh(rnd(beats * B, H, s=1.0))
    gib, ptab = rnd(beats * B, 3 * H, s=0.5), rnd(V + 1, 3 * H, s=0.5)
    mask = (torch.rand(beats * tpb, B, H, generator=g) >= 0.5).to(torch.uint8).to(dev)
    _launch3(torch, lambda: ops.tick_free_run(weights, h0a, h0b, gib, ptab, mask, 2.0, B, beats, tpb))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        ops.tick_free_run(weights, h0a, h0b, gib, ptab, mask, 2.0, B, beats, tpb)
    e1.record()
    torch.cuda.synchronize()
    print('launch (weight prep + decoder): %.1f us' % (e0.elapsed_time(e1) * 100))
    yield


def report_conv32(st, ctx):
    import numpy as np
    if ctx == 'up32p':
        return report_up32p(st)
    (tag, n), names = ctx, FAMILIES['conv32']['phases']
    tiles = n * 2
    nwg = min(256, tiles)                                # one workgroup per CU
    per_wg = max(1, min(8, -(-tiles // nwg)))
    st = st[:nwg]
    t0 = st[:, 0, 1].min()
    print(f'== {tag}: {nwg} WGs x {per_wg} tiles; whole kernel {(st[:, 63, 1].max() - t0) / 100:.1f} us (wall clock stamps)')
    cyc, wall = st[:, :, 0], st[:, :, 1]
    tot_c = (cyc[:, 63] - cyc[:, 0]).mean()
    tot_w = (wall[:, 63] - wall[:, 0]).mean()
    print(f'  WGs 0..{nwg - 1}: start {(wall[:, 0].mean() - t0) / 100:.1f} us, end {(wall[:, 63].mean() - t0) / 100:.1f} us, '
          f'span {tot_c:.0f} ticks = {tot_w / 100:.1f} us -> {tot_c / tot_w * 100:.0f} MHz')
    print('   weights', (cyc[:, 1] - cyc[:, 0]).mean().round(), ' init+first issue', (cyc[:, 2] - cyc[:, 1]).mean().round())
    for t in range(per_wg):
        s = 3 + 6 * t
        d = np.diff(cyc[:, s:s + 6], axis=1).mean(0).round()
        print('   tile', t, dict(zip(names, d.tolist())))
    print('   drain', (cyc[:, 63] - cyc[:, 3 + 6 * per_wg - 1]).mean().round())


def report_up32p(st):
    con, pro = st[:256, :, 1], st[256:, :, 1]          # consumers (thread 0), producers (thread 256): 100 MHz wall clock
    us = lambda v: v.mean() / 100  # noqa: E731
    print('compute entry -> loop start %.2f us ; whole kernel (compute waves) %.2f us, (store waves incl. last epilogue) %.2f us' %
          (us(con[:, 1] - con[:, 0]), us(con[:, 63] - con[:, 0]), us(pro[:, 63] - con[:, 0])))
    for k in range(4):
        s = 3 + 6 * k
        print('tile %d compute: request + k-loop %.2f, split next patch %.2f, wait A %.2f, handoff %.2f, wait B %.2f | store: wait A %.2f, wait B %.2f, '
              'gate request %.2f, epilogue %.2f | start %.2f us'
              % (k, us(con[:, s + 1] - con[:, s]), us(con[:, s + 2] - con[:, s + 1]), us(con[:, s + 3] - con[:, s + 2]), us(con[:, s + 4] - con[:, s + 3]),
                 us(con[:, s + 5] - con[:, s + 4]), us(pro[:, s + 1] - pro[:, s]), us(pro[:, s + 2] - pro[:, s + 1]), us(pro[:, s + 3] - pro[:, s + 2]),
                 us(pro[:, s + 4] - pro[:, s + 3]), us(con[:, s] - con[:, 0])))


def report_d32k(st, ctx):
    con, pro = st[:32], st[32:]
    print('consumer entry -> loop start: %.2f us; producer entry is %.2f us after consumer entry' %
          ((con[:, 1] - con[:, 0]).mean() / 100, (pro[:, 0] - con[:, 0]).mean() / 100))
    nt = 0
    while 8 + 5 * nt < 64 and con[0, 8 + 5 * nt] > con[0, 0]:
        nt += 1
    print('tiles per workgroup seen:', nt)
    for k in range(nt):
        c = [con[:, 5 + 5 * k] - con[:, 4 + 5 * k], con[:, 6 + 5 * k] - con[:, 5 + 5 * k], con[:, 7 + 5 * k] - con[:, 6 + 5 * k], con[:, 8 + 5 * k] - con[:, 7 + 5 * k]]
        p = [pro[:, 5 + 5 * k] - pro[:, 4 + 5 * k], pro[:, 6 + 5 * k] - pro[:, 5 + 5 * k], pro[:, 7 + 5 * k] - pro[:, 6 + 5 * k]]
        print('tile %d  consumer: k-loop %.2f, wait A %.2f, exchange + wait B %.2f, epilogue %.2f | producer: commit + loads %.2f, wait A %.2f, wait B %.2f | start %.2f us'
              % ((k,) + tuple(v.mean() / 100 for v in c) + tuple(v.mean() / 100 for v in p) + ((con[:, 4 + 5 * k] - con[:, 0]).mean() / 100,)))
    print('total %.2f us' % ((con[:, 8 + 5 * (nt - 1)] - con[:, 0]).mean() / 100))


def report_wgr(st, ctx):
    lo_sz, n = ctx
    steps = n * lo_sz * lo_sz // 32 // 256                         # steps per workgroup on 256 CUs (conv32.hip stream_geometry)
    nwg = min(256, n * lo_sz * lo_sz // 32 // steps)
    st = st[:nwg]
    c, w = st[:, 0, :, 0], st[:, 0, :, 1]
    p, pw = st[:, 1, :, 0], st[:, 1, :, 1]
    t0 = min(w[:, 0].min(), pw[:, 0].min())
    print(f'kernel span (wall stamps) {(max(w[:, 63].max(), pw[:, 63].max()) - t0) / 100:.1f} us; consumer start {(w[:,0].mean()-t0)/100:.2f} us, first barrier passed {(w[:,1].mean()-t0)/100:.2f} us, loop end {(w[:,62].mean()-t0)/100:.2f}, slab written {(w[:,63].mean()-t0)/100:.2f}')
    span_c = (c[:, 62] - c[:, 1]).mean()
    span_w = (w[:, 62] - w[:, 1]).mean()
    print(f'consumer loop: {span_c:.0f} ticks = {span_w / 100:.2f} us -> {span_c / span_w * 100:.0f} MHz; {span_c / steps:.0f} ticks per step ({steps} steps)')
    for i in range(min(steps, 16)):
        arrive, passed = c[:, 2 + 2 * i], c[:, 3 + 2 * i]
        prev = c[:, 1] if i == 0 else c[:, 3 + 2 * (i - 1)]
        pa, pb = p[:, 2 + 2 * i], p[:, 3 + 2 * i]
        print(f' step {i:2d}: consumer work {(arrive - prev).mean():6.0f}  wait at barrier {(passed - arrive).mean():6.0f} | producer issue+commit {(pb - pa).mean():6.0f}')


def report_c64s(st, ctx):
    import numpy as np
    print('entry -> loop %.2f us' % ((st[:, 1] - st[:, 0]).mean() / 100))
    for t in range(8):
        s = 2 + 6 * t
        d = np.diff(st[:, s:s + 7], axis=1).mean(0) / 100
        print('tile %d: ' % t + ', '.join('%s %.2f' % (nm, v) for nm, v in zip(FAMILIES['c64s']['phases'], d)) +
              '  | tile total %.2f' % ((st[:, s + 6] - st[:, s]).mean() / 100))


def report_midc(st, ctx):
    import numpy as np
    for pas, title in enumerate(('forward', 'backward')):
        s = st[pas]
        print(f'--- midc_{title}_kernel: first start -> last end {(s[:, 13].max() - s[:, 0].min()) / 100.0:.2f} us; per workgroup '
              f'{(s[:, 13] - s[:, 0]).mean() / 100.0:.2f} us; spread of start {(s[:, 0].max() - s[:, 0].min()) / 100.0:.2f} us')
        mean_max(FAMILIES['midc']['phases'][pas], np.diff(s[:, :14], axis=1))
        if pas == 0 and s[:, 14].any():
            print(f'   (dec0: product {(s[:, 14] - s[:, 8]).mean() / 100.0:.2f}, epilogue {(s[:, 15] - s[:, 14]).mean() / 100.0:.2f}, '
                  f'next weights issued + barrier {(s[:, 9] - s[:, 15]).mean() / 100.0:.2f} us)')


def report_mid(st, ctx):
    import numpy as np
    mean_max(FAMILIES['mid']['phases'], np.diff(st[:, :8], axis=1))
    print('total', (st[:, 7] - st[:, 0]).mean() / 100.0, 'us; spread of start', (st[:, 0].max() - st[:, 0].min()) / 100.0)


def report_rg(st, ctx):
    tag, chunks = ctx
    t0 = st[:, 0].min()
    print('== %s: workgroup start %.2f .. %.2f us after the first, end %.2f .. %.2f' % (
        tag, (st[:, 0].min() - t0) / 100, (st[:, 0].max() - t0) / 100, (st[:, 31].min() - t0) / 100, (st[:, 31].max() - t0) / 100))
    print('   entry -> loads issued %.2f us' % ((st[:, 1] - st[:, 0]).mean() / 100))
    prev = st[:, 1]
    for c in range(chunks):
        s = 2 + 5 * c
        d = [(st[:, s] - prev)] + [st[:, s + i + 1] - st[:, s + i] for i in range(4)]
        print('   chunk %d: ' % c + ', '.join('%s %.2f' % (n, v.mean() / 100) for n, v in zip(FAMILIES['rg']['phases'], d)))
        prev = st[:, s + 4]
    print('   loop end -> stores issued + drained %.2f us ; workgroup lifetime %.2f us (mean)' % (
        (st[:, 31] - st[:, 30]).mean() / 100, (st[:, 31] - st[:, 0]).mean() / 100))


def report_dw(st, ctx):
    import numpy as np
    st = st[st[:, 0] > 0]
    t0 = st[:, 0].min()
    print(len(st), 'tiles; start spread', (st[:, 0].max() - t0) / 100.0, 'us; last end', (st[:, 6].max() - t0) / 100.0, 'us')
    mean_max(FAMILIES['dw']['phases'], np.stack([st[:, b] - st[:, a] for a, b in ((0, 2), (2, 3), (3, 4), (4, 5), (5, 6))], axis=1))


# shape = (rows, slots, words per stamp) of ARVAE_STAMP_TABLE(<family>, ...) in `source` or a header it includes; view = how the
# report wants the words (default: rows x slots); phases = the names the report prints (the consumer / producer reports of d32k,
# wgr and up32p spell theirs out in their lines)
FAMILIES = {
    'conv32': dict(source='conv32.hip', flag='ARVAE_STAMPS_CONV32', shape=(512, 64, 2), view=(512, 64, 2),
                   phases=['sync', 'commit+sync', 'set_tile', 'mfma(+issue)', 'epilogue'], driver=drive_conv32, report=report_conv32),
    'd32k': dict(source='conv32.hip', flag='ARVAE_STAMPS_D32K', shape=(64, 64, 1), driver=lambda args: drive_dsprites(args, backward=False, step=False),
                 report=report_d32k),
    'wgr': dict(source='conv32.hip', flag='ARVAE_STAMPS_WGR', shape=(512, 64, 2), view=(256, 2, 64, 2), driver=drive_wgr, report=report_wgr),
    'c64s': dict(source='conv64s.hip', flag='ARVAE_STAMPS_C64S', shape=(64, 64, 1),
                 phases=['k-loop', 'w-loads + barrier', 'exchange 0', 'epilogue 0', 'exchange 1', 'epilogue 1', 'to next tile'],
                 driver=drive_c64s, report=report_c64s),
    'midc': dict(source='midcluster.hip', flag='ARVAE_STAMPS_MIDC', shape=(512, 16, 1), view=(2, 256, 16),
                 phases=[['weights issued + x0 -> LDS', 'enc0 product + slice store', 'arrive + poll (1)', 'gather (1)',
                          'enc1 product + store', 'arrive + poll (2)', 'gather (2)', 'heads + z', 'dec0',
                          'dec1 product + store + arrive + poll (3)', 'gather (3)', 'dec2 product', 'store + amax'],
                         ['weights issued + g -> LDS', 'dec2^T product + store', 'arrive + poll (1)', 'gather (1)',
                          'dec1^T product + store', 'arrive + poll (2)', 'gather (2)', 'dec0^T + d(mu, log_std)', 'heads^T',
                          'enc1^T product + store + arrive + poll (3)', 'gather (3)', 'enc0^T product', 'store + amax']],
                 driver=drive_dsprites, report=report_midc),
    'mid': dict(source='midblock.hip', flag='ARVAE_STAMPS_MID', shape=(128, 16, 1),
                phases=['touch + x0 load', 'enc fc1', 'enc fc2', 'heads + z', 'dec fc3', 'dec fc4', 'dec fc5'],
                driver=drive_dsprites, report=report_mid),
    'rg': dict(source='dense.hip', flag='ARVAE_STAMPS_RG', shape=(512, 32, 1),
               phases=['barrier', 'wait loads', 'split + LDS writes', 'barrier', 'next loads + MFMAs'], driver=drive_rg, report=report_rg),
    'dw': dict(source='dense.hip', flag='ARVAE_STAMPS_DW', shape=(512, 8, 1),
               phases=['start -> first round done', 'first round -> loop done', 'loop done -> barrier', 'partials to LDS', 'sum + stores'],
               driver=drive_dsprites, report=report_dw),
    's8': dict(source='conv64.hip', flag='ARVAE_STAMPS_S8', shape=(1, 8, 1), view=(8,),
               phases=['loop top (geometry)', 'barrier 1 (previous reads) + split + LDS writes', 'barrier 2',
                       'epilogue operands + next source requested', 'operand reads + 24 MFMAs + result tile -> LDS', 'barrier 3',
                       'epilogue: LDS reads, activation, gate, stores'], driver=drive_s8,
               report=lambda st, ctx: cycle_shares(FAMILIES['s8']['phases'], st, 'tile', f' over {st[7]} tiles (s_memtime ticks: 100 MHz -> x10 ns)')),
    'gru': dict(source='gru_seq.hip', flag='ARVAE_STAMPS_GRU', shape=(1, 5, 1), view=(5,),
                phases=[['prefetch issue + deferred stores', 'LDS operand reads + MFMAs', 'gate math + LDS writes', 'barrier'],
                        ['wait for the step operands (dh, saved gates, h_prev)', 'gate derivatives + split + LDS writes',
                         'next fetch issue + barrier', 'LDS operand reads + MFMAs + row stores + carry']],
                driver=drive_gru, report=lambda st, bwd: cycle_shares(FAMILIES['gru']['phases'][bwd], st, 'step', '' if bwd else ' (s_memtime ticks)')),
    'tick': dict(source='tick_decoder.hip', flag='ARVAE_STAMPS_TICK', shape=(1, 9, 1), view=(9,),
                 phases=['tick top: beat state / token projections requested', "layer 0 at the top (a beat's first tick only)",
                         'layer 0 gates (wait for the projections) + LDS writes', 'barrier',
                         'layer 1: operand reads + MFMAs behind the weight stream', 'layer 1 gates + LDS writes',
                         "barrier + logits / argmax + the next tick's layer 0", 'barrier + candidates -> token'],
                 driver=drive_tick, report=lambda st, ctx: cycle_shares(FAMILIES['tick']['phases'], st, 'tick')),
}


def main(argv):
    if len(argv) < 2 or argv[1] not in FAMILIES:
        sys.exit(__doc__)
    family = argv[1]
    f = FAMILIES[family]
    read = reader(family)
    for ctx in f['driver'](argv[2:]):
        f['report'](read(), ctx)


if __name__ == '__main__':
    main(sys.argv)

"""Data-parallel AR-VAE step over RCCL on real GPUs (golden G8): W ranks, each holding B/W rows
of a fixed batch, must reproduce the single-process step on the whole batch -- loss terms, the gradient every rank holds
after the all-reduce (times 1/W), and the weights after Adam.  world = 1 exercises the collectives' code path on a
one-GPU box; world = 2 needs two GPUs (skipped otherwise) and is the first test that runs RCCL between ranks.
Transport 'library' = the collectives are the library's own RCCL calls on the launch stream (arvae_comm_*, the default;
no torch process group exists in those workers); 'torch' = the same step over torch.distributed's 'nccl' group."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from arvae_amd import synthetic as syn
from oracle import image_vae as o_vae
from oracle import step as o_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_TOTAL = 64


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _failure_report(log):
    """head, every line that names an error, and tail of a failed rank's output (a HIP / RCCL error line sits in the middle
    of a long traceback: the tail alone lost it in round 3)"""
    lines = log.splitlines()
    marked = [ln for ln in lines if any(k in ln for k in ('rror', 'HIP', 'hip', 'NCCL', 'RCCL', 'abort', 'Abort', 'signal'))]
    return '\n'.join(['--- head ---'] + lines[:40] + ['--- error lines ---'] + marked[:80] + ['--- tail ---'] + lines[-60:])


def _run_ranks(world, out, capacity, fused, overlap=False, worker='dp_worker.py', args=None, transport='library'):
    port = _free_port()
    env = dict(os.environ, ARVAE_DP_OVERLAP='1' if overlap else '0', ARVAE_DP_TRANSPORT=transport)
    tail = [str(capacity), str(int(fused)), str(B_TOTAL)] if args is None else [str(a) for a in args]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', worker), str(r), str(world), str(port), out] + tail,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for r, (p, o) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, f'rank {r} exited with {p.returncode}\n' + _failure_report(o)
    return np.load(out)


# capacity 3.7 lies between the two shards' KL means of this batch (test_parallel_gloo.py): beta*|KL - c| then needs the
# all-reduced KL mean; 25 is the golden's value (dsprites_step_b8_cap_gauss uses it at B = 8)
def _needs(world, transport):
    """RCCL wants one GPU per rank; the host-staged transport (parallel.StagedComm) lets the ranks share a device"""
    if transport == 'staged':
        if world == 1:
            pytest.skip('the host-staged transport is for more ranks than GPUs')
    elif torch.cuda.device_count() < world:
        pytest.skip(f'needs {world} GPUs, this box has {torch.cuda.device_count()}')


# world 1 / 2: every transport x step form x capacity; world 4 / 8 (the SCALE run's rank counts: the gather order of eight
# row blocks, reg_scale = 8, Adam's 1/8): host-staged, ranks sharing whatever GPUs the box has
RANK_CASES = [(w, c, f, t) for w in (1, 2) for c in (0.0, 3.7) for f in (True, False) for t in ('library', 'torch', 'staged')]
RANK_CASES += [(8, 0.0, True, 'staged'), (8, 3.7, True, 'staged'), (8, 0.0, False, 'staged'), (4, 0.0, True, 'staged'),
               (8, 0.0, True, 'library'), (4, 0.0, True, 'library')]


@pytest.mark.parametrize('world,capacity,fused,transport', RANK_CASES,
                         ids=[f'{w}-{c}-{"fused" if f else "per_layer"}-{t}' for w, c, f, t in RANK_CASES])
def test_rccl_ranks_equal_single_process(tmp_path, golden_dir, world, capacity, fused, transport):
    """(transport 'staged', world >= 2: the ranks of the HIP path on whatever GPUs the box has -- all on cuda:0 on a one-GPU box --
    with the collectives staged through a gloo group on the host: the multi-rank LOGIC of the HIP path against the oracle's
    single-process step, where RCCL itself cannot run for want of more GPUs.  World 8 = BASELINE.json configs[3]'s rank count:
    8 x 8 rows against the oracle at B = 64 and the reference's golden dsprites_step_b64.npz)"""
    _needs(world, transport)
    if transport == 'torch' and not (fused and capacity == 0.0):
        pytest.skip('the torch.distributed transport is covered on the default step only')
    got = _run_ranks(world, str(tmp_path / 'dp.npz'), capacity, fused, transport=transport)
    assert int(got['world']) == world
    assert str(got['transport']) == {'library': 'LibraryComm', 'torch': 'TorchComm', 'staged': 'StagedComm'}[transport]
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    x, lab = syn.dsprites_batch(B_TOTAL, seed=1234)
    eps = syn.normal_noise((B_TOTAL, 10), seed=12)
    ref = o_step.image_step('dsprites', state, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0, capacity=capacity)
    srcs = [ref['terms']]
    if capacity == 0.0:                                        # the reference's own output for this batch (golden G4 / G8)
        srcs.append(np.load(os.path.join(golden_dir, 'dsprites_step_b64.npz')))
    for src in srcs:
        np.testing.assert_allclose(got['loss'], float(src['loss']), rtol=1e-4)
        np.testing.assert_allclose(got['acc'], float(src['acc']), rtol=1e-4)
        for k in ('recons', 'dist', 'reg'):
            np.testing.assert_allclose(got['term/' + k], float(src[k]), rtol=1e-4)
    for name in state:
        gr = got['grad/' + name].astype(np.float64).ravel()
        want = ref['grads'][name].astype(np.float64).ravel()
        assert np.linalg.norm(gr - want) <= 2e-3 * np.linalg.norm(want) + 1e-9, name
        # Adam's first step is -lr * g / (|g| + eps): an entry whose gradient is ~0 turns summation noise into a full-size
        # step, so the update is compared by its norm (as the golden tests do) and by the share of entries that moved alike
        d_got = got['param/' + name].astype(np.float64).ravel() - state[name].astype(np.float64).ravel()
        d_ref = ref['params'][name].astype(np.float64).ravel() - state[name].astype(np.float64).ravel()
        np.testing.assert_allclose(np.linalg.norm(d_got), np.linalg.norm(d_ref), rtol=2e-3, err_msg=name)
        assert (np.abs(d_got - d_ref) > 2e-5).mean() <= 2e-3, name


@pytest.mark.parametrize('world,transport', [(2, 'staged'), (2, 'library')])
def test_ranks_at_the_headline_batch_equal_single_process(tmp_path, world, transport):
    """BASELINE.json configs[3] as far as a box allows: every rank holds the HEADLINE per-GPU batch of 512 rows (global batch
    1024) -- the clustered latent block (16 clusters per rank), arvae_image_vae_finish and a regulariser whose gathered columns
    reach beyond one rank's batch, in one step -- against the oracle's single-process step on the whole batch.  'staged': both
    ranks on whatever GPUs the box has (one: they share cuda:0 -- two processes in the clustered kernels at once, as in
    tests/test_hip_parity.py::test_two_processes_share_the_device); 'library': RCCL, needs two GPUs."""
    _needs(world, transport)
    b_total = 512 * world
    got = _run_ranks(world, str(tmp_path / 'dp512.npz'), 0.0, True, transport=transport, args=[0.0, 1, b_total])
    assert int(got['world']) == world
    state = syn.synth_state(o_vae.DSPRITES_SHAPES, 1, 1.6)
    x, lab = syn.dsprites_batch(b_total, seed=1234)
    eps = syn.normal_noise((b_total, 10), seed=12)
    ref = o_step.image_step('dsprites', state, x, lab, eps, (1, 2, 3, 4, 5), 4.0, 10.0, 1.0)
    np.testing.assert_allclose(got['loss'], float(ref['terms']['loss']), rtol=1e-4)
    np.testing.assert_allclose(got['acc'], float(ref['terms']['acc']), rtol=1e-4)
    for k in ('recons', 'dist', 'reg'):
        np.testing.assert_allclose(got['term/' + k], float(ref['terms'][k]), rtol=1e-4)
    for name in state:
        gr = got['grad/' + name].astype(np.float64).ravel()
        want = ref['grads'][name].astype(np.float64).ravel()
        np.testing.assert_allclose(np.linalg.norm(gr), np.linalg.norm(want), rtol=1e-3, err_msg=name)
        assert np.linalg.norm(gr - want) <= 2e-3 * np.linalg.norm(want) + 1e-9, name
        d_got = got['param/' + name].astype(np.float64).ravel() - state[name].astype(np.float64).ravel()
        d_ref = ref['params'][name].astype(np.float64).ravel() - state[name].astype(np.float64).ravel()
        np.testing.assert_allclose(np.linalg.norm(d_got), np.linalg.norm(d_ref), rtol=2e-3, err_msg=name)


@pytest.mark.parametrize('world', [1, 2])
def test_rccl_overlapped_collectives_change_nothing(tmp_path, world):
    """the z all-gather behind the forward pass's z_ready event and the two gradient buckets all-reduced behind the backward
    pass's events on a side stream (fused.py, arvae_image_vae_t.milestones) against the same step with every collective on
    the launch stream after the pass (ARVAE_DP_OVERLAP=0): the all-reduced gradients and the weights after Adam are
    bit-identical (the same sums, only issued earlier)."""
    if torch.cuda.device_count() < world:
        pytest.skip(f'needs {world} GPUs, this box has {torch.cuda.device_count()}')
    on = _run_ranks(world, str(tmp_path / 'on.npz'), 0.0, True, overlap=True)
    off = _run_ranks(world, str(tmp_path / 'off.npz'), 0.0, True, overlap=False)
    assert float(on['loss']) == float(off['loss'])
    for k in on.files:
        if k.startswith(('grad/', 'param/')):
            np.testing.assert_array_equal(on[k], off[k], err_msg=k)


MEASURE_RANK_CASES = [(w, t, p) for p in ('executor', 'layers') for w, t in ((1, 'library'), (2, 'library'), (2, 'staged'))]
MEASURE_RANK_CASES += [(8, 'staged', 'executor'), (8, 'library', 'executor')]      # configs[4]'s rank count: 8 x 4 measures


@pytest.mark.parametrize('world,transport,path', MEASURE_RANK_CASES, ids=[f'{w}-{t}-{p}' for w, t, p in MEASURE_RANK_CASES])
def test_measure_data_parallel_step_replays_from_graphs(tmp_path, world, transport, path):
    """a data-parallel MeasureVAE step replayed from a HIP graph that holds its collective (the library's RCCL all-gather,
    recorded like the kernels around it; no torch process group, no watchdog thread in the worker) gives the eager
    data-parallel step's loss and all-reduced gradients, and those are the oracle's single-process step on the whole batch.
    Both ways the step is built: the whole-model executor (forward, grouped all-gather of z and the labels, arvae_measure_vae_finish,
    backward) and the per-layer autograd path."""
    _needs(world, transport)
    from oracle import attributes as o_attr
    from oracle import measure_vae as o_mvae
    b_total = 32
    got = _run_ranks(world, str(tmp_path / 'm.npz'), 0.0, True, worker='dp_measure_worker.py', args=[b_total, 1, path], transport=transport)
    assert int(got['world']) == world
    if transport == 'library':
        assert int(got['variants']) == 2 and str(got['transport']) == 'LibraryComm'     # one graph per teacher-forcing variant, collective inside
    else:                                       # host-staged collectives cannot be captured: the eager data-parallel step vs the oracle
        assert int(got['variants']) == 0 and str(got['transport']) == 'StagedComm'
    np.testing.assert_allclose(got['loss_replay'], got['loss_eager'], rtol=1e-6)
    ge, gr = got['grad_eager'].astype(np.float64), got['grad_replay'].astype(np.float64)
    assert np.linalg.norm(ge - gr) <= 1e-6 * np.linalg.norm(ge)
    state = syn.synth_state(o_mvae.shapes(), 4)
    score = syn.measure_batch(b_total, seed=5)
    eps = syn.normal_noise((b_total, 32), seed=1)
    attr = o_attr.attribute_labels(score, *syn.measure_tables())
    ref = o_step.measure_step(state, score, eps, attr, (0, 1, 2, 3), 0.001, 1.0, 10.0, True)
    np.testing.assert_allclose(got['loss_replay'], ref['terms']['loss'], rtol=1e-4)
    for name, (off, n) in zip(got['names'], got['spans']):
        want = ref['grads'][str(name)].astype(np.float64).ravel()
        assert np.linalg.norm(gr[off:off + n] - want) <= 3e-3 * np.linalg.norm(want) + 1e-9, name


def test_measure_data_parallel_capture_survives_repeats(tmp_path):
    """round 3's failure was intermittent (a watchdog thread polling an event while the next capture began): capture and
    replay the data-parallel step eight times in ONE process -- every capture must succeed and the last replay must still
    equal the eager step.  tools/dp_replay_loop.sh runs the worker 30 times in fresh processes."""
    got = _run_ranks(1, str(tmp_path / 'm.npz'), 0.0, True, worker='dp_measure_worker.py', args=[32, 8])
    np.testing.assert_allclose(got['loss_replay'], got['loss_eager'], rtol=1e-6)
    ge, gr = got['grad_eager'].astype(np.float64), got['grad_replay'].astype(np.float64)
    assert np.linalg.norm(ge - gr) <= 1e-6 * np.linalg.norm(ge)


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize('workload', ['dsprites', 'measure'])
def test_bench_starts_its_own_ranks(workload):
    """`python bench.py --gpus 2` without a launcher: the ranks are started by bench.py itself and rank 0's line says 2"""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    line = _bench('--gpus', '2', '--steps', '3', '--warmup', '1', '--min-seconds', '0', '--no-cpu-baseline', '--workload', workload)
    assert line['n_gpus'] == 2 and line['config']['global_batch'] == 2 * line['config']['per_gpu_batch']
    assert line['scaling'] == 'weak' and np.isfinite(line['value']) and line['value'] > 0


def test_bench_under_the_drivers_launcher_with_two_ranks():
    """the driver's command line for N = 2 -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 2 ...` -- on whatever this box has: with two GPUs over the library's RCCL communicator, with one
    GPU both ranks share it and the collectives are staged through the host (ARVAE_DP_TRANSPORT=staged).  Rank 0 prints ONE JSON
    line that says two ranks, weak scaling, twice the per-GPU batch."""
    port = _free_port()
    env = dict(os.environ)
    if torch.cuda.device_count() < 2:
        env['ARVAE_DP_TRANSPORT'] = 'staged'
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1',
                        '--min-seconds', '0', '--no-cpu-baseline', '--full'], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['scaling'] == 'weak' and line['config']['global_batch'] == 2 * line['config']['per_gpu_batch']
    assert np.isfinite(line['value']) and line['value'] > 0 and line['config']['rccl_world_size'] == 2
    assert line['config']['collectives'].startswith('StagedComm' if torch.cuda.device_count() < 2 else 'LibraryComm')
    # what the step's two exchanges cost alone (HIP events, max over ranks) and what the overlap trial decided
    dp = line['dp']
    assert dp['world'] == 2 and dp['all_reduce_us'] > 0 and dp['all_gather_us'] > 0 and 0 < dp['share_of_step']
    assert dp['grad_arena_bytes'] > 2_000_000 and ('overlap_faster' in dp['overlap_trial'] or 'error' in dp['overlap_trial'])
    assert isinstance(dp['overlap_decision'], str)


def test_bench_refuses_more_ranks_than_gpus():
    have = torch.cuda.device_count()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(have + 1), '--steps', '1', '--warmup', '0'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and f'exposes {have} GPU' in (r.stderr + r.stdout)


def test_bench_line_has_the_contract_fields():
    """--full run (short): roofline, timing, secondary workloads with their own rooflines"""
    line = _bench('--steps', '5', '--warmup', '2', '--min-seconds', '0', '--no-cpu-baseline', '--full')
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'timing', 'secondary'):
        assert k in line, k
    assert line['steps'] == 5 and line['warmup'] == 2 and line['n_gpus'] == 1 and line['vs_baseline'] is None
    rf = line['roofline']
    assert rf['bound'] in ('hbm', 'mfma') and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-9 and rf['rocprof_names']
    # the step-level fractions and every launch site of the step, each priced against ONE peak per arithmetic
    assert 0 < rf['step']['hbm_frac'] < 1 and 0 < rf['step']['flop_frac_fp32_equivalent'] < 1
    assert abs(rf['step']['ms_per_step'] - line['ms_per_step']) < 1e-9
    kernels = rf['kernels']
    assert len(kernels) >= 10 and kernels[0]['us_per_step'] >= kernels[-1]['us_per_step']
    assert abs(sum(k['share_of_device_time'] for k in kernels) - 1.0) < 1e-6
    priced = [k for k in kernels if 'frac' in k]
    assert len(priced) >= 8 and all(0 < k['frac'] < 1 and k['bound'] in ('hbm', 'mfma') for k in priced)
    assert any(k['kernel'] == rf['kernel'] and abs(k['frac'] - rf['frac']) < 1e-9 for k in priced)
    assert set(line['secondary_ms_per_step']) == {'mnist', 'measure'} and list(line).index('secondary_ms_per_step') < 10
    assert line['timing']['regions'] >= 3
    for kind in ('mnist', 'measure'):
        sec = line['secondary'][kind]
        assert 'error' not in sec, sec
        # (the fraction is of the fp32-MFMA roof; the Morpho-MNIST step multiplies on the fp16 MFMA -- three products per MAC on a pipe
        # 16x as fast -- and sits at 0.95-1.0 of the fp32 roof since round 4: not bounded by 1)
        assert sec['value'] > 0 and sec['roofline']['kernel'] and 0 < sec['step_roofline']['flop_frac_mfma16_3products'] < 1


def test_bench_plain_run_times_k_steps_and_dumps_the_same_outputs(tmp_path):
    """a plain run times exactly --steps steps, measures nothing beside the headline figure, and --dump-outputs writes what the
    last timed step computed: the same arrays from two runs with the same arguments"""
    dumps = []
    for run in ('a', 'b'):
        out = tmp_path / run
        line = _bench('--steps', '7', '--warmup', '2', '--batch', '64', '--dump-outputs', str(out))
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in line, k
        assert line['timing']['regions'] == 1 and line['timing']['steps_per_region'] == 7
        assert abs(line['value'] - 64 * 1e3 / line['ms_per_step']) <= 1e-6 * line['value']
        assert line['roofline'] is None and line['dp'] is None and 'secondary' not in line and 'cpu_baseline' not in line
        dumps.append({f.name: np.load(f) for f in sorted(out.iterdir())})
    a, b = dumps
    assert {'loss.npy', 'accuracy.npy', 'state.enc_conv.0.weight.npy', 'adam.exp_avg.npy'} <= set(a) and set(a) == set(b)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert abs(b['loss.npy'].reshape(-1)[0] - line['config']['final_loss']) <= 1e-6 * abs(line['config']['final_loss'])
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-7, err_msg=k)

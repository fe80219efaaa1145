"""The workspace contract of every entry point that takes caller-allocated memory: scratch of exactly the
reported size, arbitrary prior contents, no store outside any caller buffer.  Needs a real MI355X.

Every case of tests/workspace_cases.py runs three ways:
  (a) with the plain torch allocator -- the path the float64 suites hold;
  (b) with every torch.empty / empty_like of the product modules guarded (tests/guarded_alloc.py) and filled with 0xFF: NaN;
  (c) the same with 0x7E: 8.5e37 as fp32, finite.
Asserted: the guard bands of EVERY allocation made inside the call are intact in (b) and (c); every returned tensor and every
caller-provided accumulator (dw, db, .grad, the gradient arena, the weights after the update) is bit-identical across (a), (b) and
(c); every float result is finite; no request went past the proxy unguarded; for the executors, the optimizer's status words are
zero.  No numeric tolerance: (a) ties the guarded runs to the results the accuracy tests already judge.

The executor cases have their own test function, so the link, loss and decoder families run and report without them.  Their
arrival counters and ticket heads sit in the poisoned workspace: csrc/midprep.h clears every word of them in block 0 of the prep
launch that opens each forward call (plan.hip arvae_image_vae_forward: the prep rides in the first conv launch, in prep_all_kernel
or in mid_prep_kernel, unconditionally), before any workgroup of midcluster.hip draws a ticket, so a poisoned run behaves like a
clean one."""
import pytest
import torch

import guarded_alloc as ga
import workspace_cases as wc

pytestmark = pytest.mark.gpu

PLAIN = [c.name for c in wc.CASES if c.family != wc.EXECUTOR_FAMILY]
EXECUTORS = [c.name for c in wc.CASES if c.family == wc.EXECUTOR_FAMILY]
GUARDED_ALLOCATIONS = {}                                       # family -> guarded allocations of one poisoned run of each of its cases


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('gpu-marked test needs a GPU (the HIP path has no CPU fallback)')
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _no_launch_after_a_device_error():
    """a failing assertion lets the next case run; an error of the device itself ends the session"""
    yield
    if not torch.cuda.is_available():
        return
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, nothing further is launched: {e}', returncode=3)


def _product_modules():
    from arvae_amd import evaluation, fused, fused_measure, mnist_resnet, ops
    return ops, fused, fused_measure, evaluation, mnist_resnet


def _results(out):
    return {k: v for k, v in out.items() if not k.startswith('_')}


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _run(case, dev, monkeypatch, fill):
    """one run of the case -> (its tensors, the proxy or None); synchronised, bands checked"""
    if fill is None:
        out = case.run(dev)
        torch.cuda.synchronize()
        return _results(out), None
    with monkeypatch.context() as m:
        proxy = ga.GuardedTorch(fill).install(m, *_product_modules())
        out = case.run(dev)
        torch.cuda.synchronize()
    proxy.check_bands()
    assert proxy.passed_through == [], f'{case.name}: requests the proxy could not guard: {proxy.passed_through}'
    assert proxy.records, f'{case.name}: the case allocated nothing through the product modules'
    return _results(out), proxy


def _hold_contract(case, dev, monkeypatch):
    plain, _ = _run(case, dev, monkeypatch, None)
    nan_fill, proxy = _run(case, dev, monkeypatch, ga.FILL_NAN)
    big_fill, _ = _run(case, dev, monkeypatch, ga.FILL_BIG)
    GUARDED_ALLOCATIONS.setdefault(case.family, {})[case.name] = len(proxy.records)
    excused = {key: (site, why) for name, key, site, why in wc.EXCEPTIONS if name == case.name}
    assert set(plain) == set(nan_fill) == set(big_fill) and plain
    for key, (site, _why) in excused.items():                  # an exception names a buffer this case has and a call site it reached
        assert key in plain and site in proxy.by_site(), (case.name, key, site, sorted(proxy.by_site()))
    bad = []
    for key, want in plain.items():
        assert torch.is_tensor(want), (case.name, key)
        for how, got in (('0xFF', nan_fill[key]), ('0x7E', big_fill[key])):
            assert got.dtype == want.dtype and got.shape == want.shape, (case.name, key, how)
        if key in excused:
            print(f'{case.name} {key}: not compared ({excused[key][0]}: {excused[key][1]})')
            continue
        for how, got in (('0xFF', nan_fill[key]), ('0x7E', big_fill[key])):
            differ = int((_bits(got) != _bits(want)).sum())
            if differ:
                bad.append(f'{key}: {differ} of {_bits(want).numel()} bytes differ between the plain allocator and the {how} fill')
        if want.is_floating_point():
            for how, got in (('plain', want), ('0xFF', nan_fill[key]), ('0x7E', big_fill[key])):
                if not bool(torch.isfinite(got).all()):
                    bad.append(f'{key}: not finite under the {how} run')
    assert not bad, f'{case.name} ({len(proxy.records)} guarded allocations: {proxy.by_site()}):\n  ' + '\n  '.join(bad)
    return plain


@pytest.mark.parametrize('name', PLAIN)
def test_scratch_contract(dev, monkeypatch, name):
    _hold_contract(wc.BY_NAME[name], dev, monkeypatch)


@pytest.mark.parametrize('name', EXECUTORS)
def test_executor_scratch_contract(dev, monkeypatch, name):
    """one training step (forward, backward, optimizer.step()) or one eval forward through the trainer, noise and keep-masks pushed:
    loss, accuracy, loss terms, the gradient arena, weights and moments after the step, and the status words, which stay zero"""
    got = _hold_contract(wc.BY_NAME[name], dev, monkeypatch)
    assert not got['status'].any(), f'{name}: status words {got["status"].tolist()} (a pass failed or an update was skipped)'
    if name.endswith('train_step'):
        assert bool(got['grad_arena'].any()) and {'params', 'exp_avg', 'exp_avg_sq'} <= set(got)


def test_report_guarded_allocations_and_exceptions():
    """the figures of CHANGELOG.md: guarded allocations per family (one poisoned run of each case), and the exception list"""
    for family in wc.FAMILIES:
        per_case = GUARDED_ALLOCATIONS.get(family, {})
        print(f'{family}: {sum(per_case.values())} guarded allocations over {len(per_case)} cases')
    print(f'exceptions: {wc.EXCEPTIONS}')
    ran = {n for per_case in GUARDED_ALLOCATIONS.values() for n in per_case}
    assert ran <= set(wc.BY_NAME)

"""tests/guarded_alloc.py on CPU tensors: the proxy catches a store outside a buffer (and names the side), shows a read of an
unwritten word, passes a correct writer, and guards every request form the product modules use."""
import types

import pytest
import torch

import guarded_alloc as ga

# a "product module": its functions reach torch through the module global, as arvae_amd/ops.py does
_SOURCE = '''
import torch


def partial_sums(x, blocks, written=None, first=0):
    """sum of x through a scratch of `blocks` partials; `written` of them are stored (default: all), starting at slot `first`"""
    ws = torch.empty(blocks, dtype=x.dtype)
    written = blocks if written is None else written
    chunks = x.reshape(blocks, -1).sum(1)
    if first == 0:
        ws[:written] = chunks[:written]
    else:                                                                     # the defect: slots -1 .. blocks of the same storage
        flat = ws.as_strided((blocks + 2,), (1,), ws.storage_offset() - 1)
        flat[1 + first:1 + first + written] = chunks[:written]
    return ws.sum()


def forms(like):
    return dict(varargs=torch.empty(3, 5), tup=torch.empty((3, 5)), lst=torch.empty([2, 2], dtype=torch.float64),
                size=torch.empty(torch.Size((4,)), dtype=torch.int64), kw=torch.empty(size=(2, 3), dtype=torch.uint8),
                scalar=torch.empty((), dtype=torch.float32), zero=torch.empty(0, dtype=torch.float32),
                zero2d=torch.empty(3, 0, 4, dtype=torch.int32), like=torch.empty_like(like),
                like_dtype=torch.empty_like(like, dtype=torch.int64), half=torch.empty(7, dtype=torch.float16),
                grad=torch.empty(2, 2, requires_grad=True))


def unguardable(like):
    return torch.empty_like(like.t()), torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
'''


@pytest.fixture
def product():
    mod = types.ModuleType('fake_product')
    exec(compile(_SOURCE, 'fake_product.py', 'exec'), mod.__dict__)
    assert mod.torch is torch
    return mod


def _x(dtype=torch.float32):
    return torch.arange(1, 33, dtype=dtype) / 8


@pytest.mark.parametrize('fill', [ga.FILL_NAN, ga.FILL_BIG])
def test_a_correct_writer_and_consumer_pass_both_checks(product, monkeypatch, fill):
    want = product.partial_sums(_x(), 4)
    g = ga.GuardedTorch(fill).install(monkeypatch, product)
    got = product.partial_sums(_x(), 4)
    g.check_bands()
    assert got.view(torch.int32) == want.view(torch.int32)
    assert len(g.records) == 1 and g.passed_through == []
    rec = g.records[0]
    assert rec.site.startswith('fake_product.py:') and 'partial_sums' in rec.site
    assert rec.dtype == torch.float32 and rec.shape == (4,) and rec.base.numel() == 2 * ga.GUARD + 16


@pytest.mark.parametrize('first, side, where', [(1, 'after', +0), (-1, 'before', -1)])
def test_one_element_outside_the_buffer_fails_with_the_side_named(product, monkeypatch, first, side, where):
    g = ga.GuardedTorch(ga.FILL_NAN).install(monkeypatch, product)
    product.partial_sums(_x(), 4, first=first)
    (rec, got_side, offset, count), = g.damaged()
    assert got_side == side and offset == where and 1 <= count <= 4 and 'partial_sums' in rec.site
    with pytest.raises(AssertionError, match=rf'written {side} the buffer allocated at fake_product\.py:\d+ \(partial_sums\)'):
        g.check_bands()


def test_an_unwritten_word_shows_as_different_bytes_and_as_non_finite_under_the_nan_fill(product, monkeypatch):
    out = {}
    for fill in (ga.FILL_NAN, ga.FILL_BIG):
        with monkeypatch.context() as m:
            g = ga.GuardedTorch(fill).install(m, product)
            out[fill] = product.partial_sums(_x(), 4, written=3)
            g.check_bands()
    assert product.torch is torch
    assert not torch.isfinite(out[ga.FILL_NAN])
    assert out[ga.FILL_NAN].view(torch.int32) != out[ga.FILL_BIG].view(torch.int32)
    want = _x()[:24].sum()
    assert torch.isfinite(out[ga.FILL_BIG]) and abs(out[ga.FILL_BIG] - want) > 1e30        # 0x7E7E7E7E = 8.5e37 drowns the sum


def test_every_request_form_is_guarded(product, monkeypatch):
    like = torch.zeros(2, 3, dtype=torch.float64)
    plain = product.forms(like)
    g = ga.GuardedTorch(ga.FILL_NAN).install(monkeypatch, product)
    got = product.forms(like)
    g.check_bands()
    assert g.passed_through == [] and len(g.records) == len(got)
    for name, t in got.items():
        p = plain[name]
        assert (t.shape, t.dtype, t.device, t.stride(), t.requires_grad) == (p.shape, p.dtype, p.device, p.stride(), p.requires_grad), name
        assert t.is_contiguous() and not t._is_view() and t.data_ptr() % 16 == 0, name
        if t.numel():
            assert t.is_floating_point() and bool(t.isnan().all()) or not t.is_floating_point() and bool((t.view(torch.uint8) == 0xFF).all()), name
        t.detach().fill_(1)                                             # the whole middle is writable ...
    g.check_bands()                                                     # ... and writing all of it leaves the bands alone
    assert got['size'].tolist() == [1] * 4
    sizes = {r.shape: r.nbytes for r in g.records}
    assert sizes[()] == 4 and sizes[(0,)] == 0 and sizes[(3, 0, 4)] == 0 and sizes[(7,)] == 14


def test_integers_read_minus_one_and_fp32_reads_the_big_finite_value(product, monkeypatch):
    g = ga.GuardedTorch(ga.FILL_BIG).install(monkeypatch, product)
    t = product.torch.empty(3)
    assert t.tolist() == [torch.tensor([0x7E7E7E7E], dtype=torch.int32).view(torch.float32).item()] * 3 and 8e37 < t[0] < 9e37
    monkeypatch.setattr(product, 'torch', torch)
    g = ga.GuardedTorch(ga.FILL_NAN).install(monkeypatch, product)
    assert product.torch.empty(2, dtype=torch.int64).tolist() == [-1, -1]
    assert product.torch.empty(2, dtype=torch.uint8).tolist() == [255, 255]


def test_what_cannot_be_guarded_is_passed_through_and_counted(product, monkeypatch):
    g = ga.GuardedTorch(ga.FILL_NAN).install(monkeypatch, product)
    a, b = product.unguardable(torch.zeros(3, 4))
    assert a.shape == (4, 3) and b.is_contiguous(memory_format=torch.channels_last)
    assert len(g.passed_through) == 2 and g.records == []
    assert all(site.startswith('fake_product.py:') for site, _ in g.passed_through)


def test_everything_else_is_the_real_torch(product, monkeypatch):
    g = ga.GuardedTorch(ga.FILL_NAN).install(monkeypatch, product)
    assert g.zeros is torch.zeros and g.float32 is torch.float32 and g.Tensor is torch.Tensor and g.cuda is torch.cuda
    with pytest.raises(AttributeError):
        g.empty = None
    with pytest.raises(AssertionError):
        g.install(monkeypatch, product)                                 # already patched: no module-global real torch

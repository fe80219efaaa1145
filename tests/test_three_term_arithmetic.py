"""CPU model of the three-term bf16 arithmetic (ar-vae_amd/csrc/splitmath.h: split3 and X3_MFMA6) next to the two-term fp16 model
(test_two_term_arithmetic.py), and the proof that the bar of test_split_kernels_float64.py tells a right kernel from a wrong one.

split3: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round-to-nearest-even (torch.bfloat16 rounds the same way);
a multiply-add is the six partial products lo hi', hi lo', mid mid', mid hi', hi mid', hi hi' (each exact in fp32: 8 x 8 bits),
accumulated in fp32.  As in the two-term model the accumulation is modelled in float64 and rounded once: what the kernels add
on top is the fp32 summation's own error, which the sequential chain below bounds from above."""
import numpy as np
import pytest
import torch

from split_cases import FLOOR, R, reduction_lengths
from test_two_term_arithmetic import rel, split

PRODUCTS6 = {'lh': (2, 0), 'hl': (0, 2), 'mm': (1, 1), 'mh': (1, 0), 'hm': (0, 1), 'hh': (0, 0)}      # X3_MFMA6's order


def split3(x):
    """splitmath.h split3 on an fp32 array -> (hi, mid, lo) as float64 arrays holding bf16 values"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    hi = t.bfloat16().float()
    r = t - hi                                           # exact in fp32
    mid = r.bfloat16().float()
    q = r - mid                                          # exact in fp32
    lo = q.bfloat16().float()
    return tuple(v.double().numpy() for v in (hi, mid, lo))


def matmul_three_term(a, b, drop=None):
    """[M, K] x [K, N] on the six products (without the one named by `drop`), accumulated exactly, rounded once"""
    sa, sb = split3(a), split3(b)
    acc = sum(sa[i] @ sb[j] for name, (i, j) in PRODUCTS6.items() if name != drop)
    return acc.astype(np.float32)


def matmul_two_term(a, b, drop=None):
    """test_two_term_arithmetic.matmul_two_term with one of the products l h' ('lh'), h l' ('hl') left out on request"""
    ah, al, _sa, ia = split(a)
    bh, bl, _sb, ib = split(b)
    f = np.float64
    terms = {'lh': al.astype(f) @ bh.astype(f), 'hl': ah.astype(f) @ bl.astype(f), 'hh': ah.astype(f) @ bh.astype(f)}
    acc = sum(v for name, v in terms.items() if name != drop)
    return (acc * f(ia) * f(ib)).astype(np.float32)


def fp32_chain(a, b):
    """a sequential fp32 multiply-add chain over the whole reduction: the worst summation order a correct fp32-accumulating
    kernel could have (every kernel here splits the reduction over waves, slices or MFMA rows, i.e. has shorter chains)"""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * b[k:k + 1, :]
    return acc


def test_three_terms_reproduce_an_fp32_value_to_2_pow_minus_26():
    rs = np.random.RandomState(0)
    x = (rs.standard_normal(1 << 16) * np.exp(2.0 * rs.standard_normal(1 << 16))).astype(np.float32)
    hi, mid, lo = split3(x)
    err = np.abs(hi + mid + lo - x.astype(np.float64))
    assert np.all(err <= np.abs(x) * 2.0 ** -26)
    assert np.all(np.abs(mid) <= np.abs(x) * 2.0 ** -8) and np.all(np.abs(lo) <= np.abs(x) * 2.0 ** -16)
    # each term has 8 significant bits: a product of two terms is exact in fp32
    for t in (hi, mid, lo):
        assert np.array_equal(torch.from_numpy(t).bfloat16().double().numpy(), t)


def test_six_products_sit_at_fp32_rounding_noise_and_every_one_of_them_is_needed():
    rs = np.random.RandomState(1)
    a = rs.standard_normal((256, 1024)).astype(np.float32)
    b = (rs.standard_normal((1024, 64)) * 0.2).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    e_six = rel(matmul_three_term(a, b), ref)
    assert e_six < 2.0 ** -24, e_six                     # one rounding to fp32 (at most 2^-24 of each value), nothing else visible
    for drop in ('lh', 'hl', 'mm', 'mh', 'hm'):
        assert rel(matmul_three_term(a, b, drop), ref) > 30 * e_six, drop
    # power-of-two scaling changes nothing but the exponent (bf16 has fp32's exponent range: no scale to carry)
    got = matmul_three_term(a * np.float32(2.0 ** -23), b * np.float32(2.0 ** 9))
    np.testing.assert_array_equal(got, matmul_three_term(a, b) * np.float32(2.0 ** -14))


@pytest.mark.parametrize('k', reduction_lengths())
def test_the_float64_bar_separates_a_missing_product_from_fp32_summation_noise(k):
    """For every reduction length of the GPU table (split_cases.py), with the data of its cases (N(0,1) activations, weights
    x 0.2): the bar R * e_cpu + FLOOR lies above the error of a sequential fp32 chain over the whole reduction (b) and below
    the error of every 'one product missing' variant of the six-product bf16 and the three-product fp16 arithmetic (a).
    e_cpu is torch's fp32 CPU matrix product, as in the GPU test."""
    rs = np.random.RandomState(k)
    m, n = 128, 64
    a = rs.standard_normal((m, k)).astype(np.float32)
    b = (rs.standard_normal((k, n)) * 0.2).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    e_cpu = rel((torch.from_numpy(a) @ torch.from_numpy(b)).numpy(), ref)
    bar = R * e_cpu + FLOOR
    e_chain = rel(fp32_chain(a, b), ref)
    wrong = {f'bf16x3 without {d}': rel(matmul_three_term(a, b, d), ref) for d in ('lh', 'hl', 'mm', 'mh', 'hm')}
    wrong.update({f'fp16x2 without {d}': rel(matmul_two_term(a, b, d), ref) for d in ('lh', 'hl')})
    right = {'bf16x3': rel(matmul_three_term(a, b), ref), 'fp16x2': rel(matmul_two_term(a, b), ref), 'fp32 chain': e_chain}
    print(f'K={k}: e_cpu {e_cpu:.2e}  bar {bar:.2e}  chain {e_chain:.2e} ({e_chain / e_cpu:.2f} x)  '
          f'least missing product {min(wrong.values()):.2e} ({min(wrong.values()) / e_cpu:.2f} x)')
    for name, e in right.items():
        assert e < bar, (name, e, bar)
    for name, e in wrong.items():
        assert e > bar, (name, e, bar)

"""CPU proof for the float64 tests of the 32 <-> 32 channel links (conv32_cases.py, test_conv32_links_float64.py):

  1. the two float64 references (torch, and numpy by im2col / einsum / col2im) agree to 1e-12 relative at every case, and the fp32
     yardstick passes both forms of the bar;
  2. the host code of conv32.hip restated (launch()): at cus = 256 every row of the threshold table has cases on both sides of its
     threshold and a partial-tile case where it can have one, and every case's `kernel` is the variant the host code picks;
  3. the CPU model of the kernels' arithmetic (the scaled two-term fp16 product of test_two_term_arithmetic.py on the case's own
     im2col matrices) passes both forms of the bar at every case, figures printed;
  4. the table is sharp: every wrong kernel of WRONG_KERNELS fails the bar at each case that reaches its edge and passes the cases
     of the same kernels that do not.

Runs anywhere (no GPU)."""
import zlib

import numpy as np
import pytest
import torch

import conv32_cases as cc
import test_two_term_arithmetic as tt

CASES = {cc.case_id(c): c for c in cc.CASES}
CONV32 = [cid for cid, c in CASES.items() if c.kernel != cc.GENERIC]


def _quiet(*_a):
    pass


@pytest.fixture(scope='module')
def computed():
    """inputs and the two torch results of a case, computed once and kept while consecutive tests ask for the same case"""
    last = {}

    def get(cid):
        if last.get('id') != cid:
            last.clear()
            case = CASES[cid]
            t = cc.inputs(case)
            last.update(id=cid, case=case, t=t, ref=cc.maps_torch(case, t, torch.float64), cpu=cc.maps_torch(case, t, torch.float32))
        return last['case'], last['t'], last['ref'], last['cpu']
    return get


# ---------------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize('cid', list(CASES))
def test_references_agree_and_the_yardstick_passes(computed, cid):
    case, t, ref, cpu = computed(cid)
    other = cc.maps_numpy(case, t)
    assert set(ref) == set(other) == set(cc.wants(case))
    for k in ref:
        assert ref[k].shape == np.shape(other[k]) and ref[k].dtype == np.float64 and cpu[k].dtype == np.float32, k
        assert cc.rel(other[k], ref[k]) <= 1e-12, (k, cc.rel(other[k], ref[k]))
        if k in ('down', 'up'):
            assert cc.rel_images(other[k], ref[k]).max() <= 1e-12, k
    assert not cc.hold(cid, cpu, cpu, ref, say=_quiet)


def test_ids_are_unique_and_seeds_are_the_crc32_of_the_id():
    assert len(CASES) == len(cc.CASES)
    for cid, case in CASES.items():
        a, b = cc._rs(case).standard_normal(4), np.random.RandomState(zlib.crc32(cid.encode()) & 0x7fffffff).standard_normal(4)
        assert a.tobytes() == b.tobytes(), cid
    t = cc.inputs(cc.WGRAD_CASES[3])
    again = cc.inputs(cc.WGRAD_CASES[3])
    assert all(np.array_equal(t[k], again[k]) for k in t)
    assert np.abs(t['dw0']).min() > 0 and np.abs(t['db0']).min() > 0             # an accumulating case starts from non-zero values


def test_amax_tail_inputs():
    """the tail cases: the largest magnitude is 64 x the rest and lies in the last 16 bytes; one per route at a partial tile"""
    tails = [c for c in cc.CASES if c.amax_tail]
    assert {c.route for c in tails} == {'down', 'up', 'wgrad'}
    for c in tails:
        x = cc.inputs(c)[c.amax_tail].reshape(-1)
        assert int(np.argmax(np.abs(x))) >= x.size - 4 and np.abs(x).max() == 64 * np.abs(np.delete(x, np.argmax(np.abs(x)))).max()
        la = cc.launch(c.route, c.lo, cc.batch(c))
        assert cc.batch(c) % la.ti != 0 or (la.tiles % la.per_wg != 0 and la.per_wg > 2), cc.case_id(c)


# ---------------------------------------------------------------------------------------------------------------- 2. the host code
def test_tile_geometry_is_conv32_commons():
    """Tile<LO, PX> as conv32_common.h lists it"""
    assert cc.tile_images(16, 128) == (1, 8) and cc.tile_images(8, 128) == (2, 8) and cc.tile_images(4, 128) == (8, 4)
    assert cc.tile_images(4, 32) == (2, 4) and cc.tile_images(16, 64) == (1, 4) and cc.tile_images(8, 64) == (1, 8)
    assert cc.tile_images(8, 32) == (1, 4) and cc.tile_images(4, 64) == (4, 4)


# the issue's threshold table at cus = 256: (route, lo, kernel) -> (tiles of n, first batch of the second pass or None when every
# batch of the variant is in it, images per tile, the batches the table must hold)
THRESHOLDS = {
    ('down', 16, cc.D16): (lambda n: 4 * n, 65, 1, (1, 3, 64, 65, 130)),
    ('down', 8, cc.D8): (lambda n: n, 257, 1, (1, 3, 256, 257)),
    ('down', 4, cc.D4): (lambda n: -(-n // 2), 1025, 2, (1, 3, 1024, 1025)),
    ('up', 16, cc.U16): (lambda n: 2 * n, 129, 1, (1, 3, 128, 129)),
    ('up', 8, cc.U8S): (lambda n: 2 * n, 129, 1, (1, 3, 128, 129, 512)),
    ('up', 8, cc.U8L): (lambda n: -(-n // 2), None, 2, (513, 514)),
    ('up', 4, cc.U4S): (lambda n: -(-n // 2), 513, 2, (1, 3, 512, 513, 1024)),
    ('up', 4, cc.U4L): (lambda n: -(-n // 8), 2049, 8, (1025, 2048, 2049)),
    ('wgrad', 4, cc.W4): (lambda n: -(-n // 4), 1025, 4, (1, 2, 3, 4, 5, 1024, 1025)),
}


def test_every_case_names_the_kernel_the_host_code_picks():
    for cid, c in CASES.items():
        if c.kernel == cc.GENERIC:
            assert c.outside or c.act == 'selu' or c.lo == 2, cid          # one step outside conv32_fits / the per-layer predicates
            continue
        assert c.lo in (16, 8, 4) and c.act in ('none', 'relu') and not c.outside
        la = cc.launch(c.route, c.lo, cc.batch(c))
        assert la.kernel == c.kernel, (cid, la)
        assert c.kernel in cid and f'-n{cc.batch(c)}' in cid              # batch and kernel name in the collected test id
        if (c.route, c.lo, c.kernel) in THRESHOLDS:
            assert la.tiles == THRESHOLDS[c.route, c.lo, c.kernel][0](cc.batch(c)), cid
    # the variant switches of launch_up_v: n <= 2 cus / 4 cus on 32-pixel tiles, above on 128
    assert cc.launch('up', 8, 512).px == 32 and cc.launch('up', 8, 513).px == 128
    assert cc.launch('up', 4, 1024).px == 32 and cc.launch('up', 4, 1025).px == 128
    assert cc.launch('down', 4, 1024).grid == 512 and cc.launch('down', 4, 1025).grid == 512          # down_small_grid: 2 cus
    assert cc.launch('wgrad', 16, 37).per_wg == 2 and cc.launch('wgrad', 8, 37).per_wg == 1           # stream_geometry


@pytest.mark.parametrize('row', list(THRESHOLDS), ids=lambda r: f'{r[0]}{r[1]}-{r[2]}')
def test_threshold_table_has_cases_on_both_sides(row):
    route, lo, kernel = row
    _tiles, second, ti, batches = THRESHOLDS[row]
    mine = [c for c in cc.CASES if (c.route, c.lo, c.kernel) == row]
    have = {cc.batch(c) for c in mine}
    assert set(batches) <= have, (row, sorted(have))
    passes = {n: cc.launch(route, lo, n).per_wg for n in have}
    if second is None:                                                     # every batch of the variant is past the single pass
        assert all(p > 1 for p in passes.values())
        first = min(have)
        assert cc.launch(route, lo, first - 1).kernel != kernel            # ... and the table holds the variant's first batch
    else:
        assert passes[second - 1] == 1 and passes[second] == 2             # the last batch of the single pass, the first of the second
        assert cc.launch(route, lo, second - 1).kernel == kernel == cc.launch(route, lo, second).kernel
    if min(batches) == 1:
        assert 1 in have and any(n % 2 == 1 and 1 < n < 8 for n in have)   # n = 1 and a small odd n
    if ti > 1:
        assert any(n % ti != 0 for n in have) and any(n % ti == 0 for n in have)          # a partial last tile, and none
    if row == ('down', 16, cc.D16):                                        # the runs that start inside an image
        la = cc.launch('down', 16, 130)
        assert la.per_wg == 3 and la.per_wg % 4 != 0 and la.tiles % la.per_wg != 0


def test_wgrad_table_holds_what_the_row_stream_test_leaves_out():
    w = [c for c in cc.WGRAD_CASES]
    for lo in (16, 8):
        assert {cc.batch(c) for c in w if c.lo == lo and c.bias_side == 0} >= {3, 37}
    for lo in (16, 8, 4):
        assert any(c.accumulate for c in w if c.lo == lo)
    for n in (3, 5):
        assert {c.bias_side for c in w if c.lo == 4 and cc.batch(c) == n} == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------- 3. the model
def test_local_two_term_product_is_matmul_two_term():
    rs = np.random.RandomState(3)
    a, b = rs.standard_normal((96, 128)).astype(np.float32), (rs.standard_normal((128, 32)) * 0.1).astype(np.float32)
    want = tt.matmul_two_term(a, b)
    assert cc._two_term(a, b, np.abs(a).max(), np.abs(b).max()).tobytes() == want.tobytes()
    pa, pb = cc._pinned(a, b[:64].repeat(2, 0) * 0.25, np.abs(b).max())          # a smaller b under the whole tensor's scale
    assert tt.matmul_two_term(pa, pb).tobytes() == cc._two_term(pa[:, :-1], pb[:-1], np.abs(a).max(), np.abs(b).max()).tobytes()
    assert cc.rel(cc._two_term(a, b, np.abs(a).max(), np.abs(b).max(), drop_lh=True), want.astype(np.float64)) > 1e-5


@pytest.mark.parametrize('cid', CONV32)
def test_the_model_passes(computed, cid):
    case, t, ref, cpu = computed(cid)
    bad = cc.hold(cid, cc.model(case, t), cpu, ref)
    assert not bad, (cid, bad)


# ---------------------------------------------------------------------------------------------------------------- 4. sharpness
def test_every_wrong_kernel_has_cases_on_both_sides():
    """statically: each defect applies somewhere and reaches its edge somewhere; the ones with an edge the small cases do not
    reach also have a case that stays inside, in every kernel they apply to"""
    for name, (_fn, applies, reaches) in cc.WRONG_KERNELS.items():
        mine = [c for c in cc.CASES if applies(c)]
        assert any(reaches(c) for c in mine), name
        if name[0] in 'abcfg':
            for kernel in {c.kernel for c in mine}:
                of = [c for c in mine if c.kernel == kernel]
                if name[0] == 'a' and kernel == cc.U8L:
                    assert all(reaches(c) for c in of)                     # (128-pixel tiles at 8 x 8 start past the single pass)
                    continue
                if name[0] == 'g' and not any(c.amax_tail for c in of):
                    continue
                assert any(reaches(c) for c in of) and any(not reaches(c) for c in of), (name, kernel)
    names = ' '.join(cc.WRONG_KERNELS)
    for word in ('first pass', 'partial tile dropped', 'first image', 'adjacent pixel', 'l h\'', 'overwrites', 'scale', 'before the bias'):
        assert word in names, word


@pytest.mark.parametrize('cid', CONV32)
def test_wrong_kernels_fail_exactly_where_their_edge_is_reached(computed, cid):
    case, t, ref, cpu = computed(cid)
    for name, (_fn, applies, reaches) in cc.WRONG_KERNELS.items():
        if not applies(case):
            continue
        bad = cc.hold(f'{cid} [{name}]', cc.wrong_kernel(name, case, t), cpu, ref)
        assert bool(bad) == bool(reaches(case)), (cid, name, 'fails' if bad else 'passes', bad)


def test_one_damaged_image_among_513_is_seen_by_the_per_image_form_alone():
    """what the per-image form adds: the last image of up 8 x 8 at n = 513 a relative 2e-6 off (two dozen fp32 ulps) passes the
    whole-tensor bar and fails its own"""
    cid = next(i for i, c in CASES.items() if c.kernel == cc.U8L and cc.batch(c) == 513 and not c.amax_tail)
    case = CASES[cid]
    t = cc.inputs(case)
    ref, cpu = cc.maps_torch(case, t, torch.float64), cc.maps_torch(case, t, torch.float32)
    got = cc.model(case, t)
    got['up'][-1] *= np.float32(1 + 2e-6)
    bad = cc.hold(cid, got, cpu, ref)
    assert [b[1] for b in bad] == ['images'] and bad[0][2] == [512], bad

"""The integer inputs of tests/test_gpu_dense_exact.py (tests/exact_dense.py), checked on the CPU -- so that a failure
on the device is never the test's own arithmetic: the row means are exact integers, everything stays below 2^53, and the
float64 BLAS product the device is compared with IS the int64 product.  And the restated dispatch gives every case the
kernel, the slabs per workgroup and the ragged end it is there for."""
import numpy as np
import pytest

import exact_dense as ed

N_HOST, ROWS_HOST = 272, 2087              # one small shape: 17 tiles a side, a last slab of 7 rows


def test_row_means_are_exact_integers_and_float64_is_int64():
    X = ed.gram_case(N_HOST, ROWS_HOST)
    c = ed.xb_case(N_HOST, ROWS_HOST)
    for M in (X, c['X'], c['W'], c['W5'], c['M'], c['M2']):
        np.testing.assert_array_equal(M, np.rint(M))
    Xi = X.astype(np.int64)
    assert np.abs(Xi[:, :-1]).max() <= 8 + 3 and len(np.unique(Xi)) > 17
    # the mean as the kernels take it: the row sum (integers: exact in any order) over N, one division
    Xb, m = c['X'], c['m']
    np.testing.assert_array_equal(Xb.sum(axis=1) / N_HOST, m)
    np.testing.assert_array_equal(Xb[:, ::-1].sum(axis=1) / N_HOST, m)
    assert np.abs(m).max() <= 3 and len(np.unique(m)) == 7
    np.testing.assert_array_equal(Xb - m[:, None], np.rint(Xb - m[:, None]))
    # X^T X: bound, float64 == int64, and in the opposite order of the rows
    want = X.T @ X
    assert np.abs(want).max() < ed.LIMIT and np.abs(want).max() == want.diagonal().max()
    np.testing.assert_array_equal(want, (Xi.T @ Xi).astype(np.float64))
    np.testing.assert_array_equal(want, X[::-1].T @ X[::-1])
    np.testing.assert_array_equal(want, want.T)
    # X . W and the two residualisations: bound, float64 == int64
    Xc = Xb - m[:, None]
    assert ed.xb_bound(Xb, c['W']) < ed.LIMIT and ed.xb_bound(Xc, c['M'].T, c['M2'].T) < ed.LIMIT
    Xci, Mi, M2i = Xc.astype(np.int64), c['M'].astype(np.int64), c['M2'].astype(np.int64)
    np.testing.assert_array_equal(Xb @ c['W'], (Xb.astype(np.int64) @ c['W'].astype(np.int64)).astype(np.float64))
    np.testing.assert_array_equal(Xb @ c['W5'], (Xb.astype(np.int64) @ c['W5'].astype(np.int64)).astype(np.float64))
    np.testing.assert_array_equal(Xc @ c['M'].T @ c['M2'].T, (Xci @ Mi.T @ M2i.T).astype(np.float64))
    for M in (c['W'], c['M'], c['M2']):
        assert np.abs(M).max() <= 3 and not np.array_equal(M, M.T)
    # the poison: same width, 64 more rows, large enough to change any sum it enters and still exact
    P = ed.poison(ROWS_HOST, N_HOST)
    assert P.shape == (ROWS_HOST + 64, N_HOST) and (P == 2.0 ** 20).all()
    assert np.abs(want).max() + ed.POISON_ROWS * ed.POISON ** 2 < ed.LIMIT


@pytest.mark.parametrize('N,n,blk_small,kernel,cap,slab,slabs,passes', ed.GRAM_CASES)
def test_gram_cases_make_a_workgroup_loop(N, n, blk_small, kernel, cap, slab, slabs, passes):
    p = ed.gram_plan(n, N, bool(blk_small))
    assert (p['kernel'], p['cap'], p['slab'], p['slabs'], p['passes']) == (kernel, cap, slab, slabs, passes)
    assert n == ed.loop_rows(cap, slab, slabs) and p['nblocks'] == cap and p['last_rows'] == 7
    # three slabs where a second buffer is filled under the MFMAs (both buffers written twice), two in the single buffer
    assert slabs == (2 if kernel.startswith('k_gram<') else 3)
    # workgroups 0 ... 5 walk `slabs` slabs, and the ragged one is the last slab of workgroup 5
    assert p['nslab'] - cap * (slabs - 1) == 6
    assert 8 * (n + ed.POISON_ROWS) * p['ldx'] < 80e6                     # (an upload stays under 80 MB)


def test_gram_cases_cover_the_families_and_strides():
    kernels = {c[3] for c in ed.GRAM_CASES}
    assert {'k_gram_blk<4>', 'k_gram_blk<8>', 'k_gram_blk<12>', 'k_gram_blk<16>', 'k_gram_db<1>', 'k_gram_db<2>',
            'k_gram_db<3>', 'k_gram_db<4>', 'k_gram_db<9>', 'k_gram<9,16,32>', 'k_gram<9,16,16>'} == kernels
    assert [ed.x_ld(N) for N in (96, 144, 160, 200, 240, 256, 272)] == [96, 144, 164, 200, 240, 256, 272]
    # the thresholds between the families: two slabs in LDS up to 272 samples, 32-row slabs up to 592
    assert ed.gram_plan(16551, 273)['kernel'] == 'k_gram<9,16,32>'
    assert ed.gram_plan(16551, 592)['slab'] == 32 and ed.gram_plan(16551, 593)['kernel'] == 'k_gram<9,16,16>'
    for N, n in ed.GRAM_SMALL:
        p = ed.gram_plan(n, N)
        assert p['slabs'] == 1 and p['nblocks'] == p['nslab'] <= 3


@pytest.mark.parametrize('N,n,kernel,tiles', ed.XB_CASES)
def test_xb_cases_reach_their_kernels(N, n, kernel, tiles):
    p = ed.xb_plan(n, N, N)
    assert (p['kernel'], p['tiles']) == (kernel, tiles)
    if kernel.startswith('k_xb_res'):
        assert p['ntile'] >= 65 and p['last_rows'] < 16 and p['strips'] == (2 if N > 64 else 1)
        assert ed.xb_plan(n, N, 5)['kernel'] == kernel
    if tiles == 2:                            # six waves of the first workgroup come round again; the last tile is ragged
        assert p['ntile'] - 512 * 16 == 6 and p['last_rows'] == 3

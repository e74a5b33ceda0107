"""X^T X and X . B on inputs where they have ONE right answer, at the shapes where a workgroup LOOPS (run with -m gpu on
an MI355X).

tests/exact_dense.py: integer-valued X with exactly integer row means, integer B / M / W, every partial sum an integer
below 2^53 -- the MFMA chains, k_gram_reduce and the float64 BLAS reference give the same bits in any order, so every
comparison is array_equal (tests/test_dense_exact_host.py checks the builder, the bound and float64 == int64 on the
CPU).  Ahead of every case a matrix of 2^20 with 64 more rows is uploaded: the X buffer only grows, so a kernel that
reads past the last row in its last slab or tile changes an integer.

X^T X (mfma.hip:gram_plan, launch_gram_range, launch_gram_t; exact_dense.gram_plan restates them and the cases assert
it).  n = cap . slab . (slabs - 1) + 5 slab + 7: workgroups 0 ... 5 walk `slabs` slabs, the last slab holds 7 rows.

  N     kernel                                    cap x slab   n      slabs per workgroup
  48    k_gram_db<1>                              512 x 32     32935  3
  80    k_gram_db<1>  (5 tiles a side: no blocks) 512 x 32     32935  3
  96    k_gram_blk<4, PF 6>, ldx = 96             512 x 32     32935  3   (two workgroups per CU)
  144   k_gram_blk<8>                             512 x 32     32935  3   (two workgroups per CU)
  160   k_gram_blk<12>, ldx = 164                 256 x 32     16551  3
  200   k_gram_blk<16>, ldx = 200                 256 x 32     16551  3
  240   k_gram_blk<16>, ldx = 240                 256 x 32     16551  3
  256   k_gram_db<9>, one grid.y pass             512 x 32     32935  3
  272   k_gram_db<9>, two passes                  512 x 32     32935  3
  300   k_gram<9,16,32> single buffer, 2 passes   512 x 32     16551  2
  576   k_gram<9,16,32>, 5 passes (LDS limit)     512 x 32     16551  2
  640   k_gram<9,16,16>, 6 passes                 512 x 16     8279   2
  1024  k_gram<9,16,16>, 15 passes                252 x 16     4119   2   (cap: partial tiles under 1 GiB)
  96 / 144 / 160 with CNA_GRAM_BLK_SMALL=0:
        k_gram_db<2> / <3> / <4>                  512 x 32     32935  3
  n = 1, 31, 33 at N = 48, 96, 200, 640: fewer rows than a slab (or one row in the second): `lim` on the first load.

X . B (mfma.hip:launch_xb; exact_dense.xb_plan): project(W) with W N x N and N x 5, then resid_apply(M, centre) and
resid_apply(M2, no centre) in place.

  N = 4, 50, 100, 128 at n = 1029   65 tiles: k_xb_res (B resident; two 4-tile strips of B from 65 columns on)
  the same at n = 1008              63 tiles: k_xb<., 4>
  N = 8 at n = 131155               8198 tiles on 512 x 16 waves: six waves take a second tile, the last holds 3 rows
  N = 132, 256 at n = 1029          k_xb<33,2>, k_xb<64,2>
  N = 260, 520 at n = 1029          the k-split (64 + 1 and 64 + 64 + 2 quads) with k_row_means, into a second buffer
"""
import numpy as np
import pytest

import exact_dense as ed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    return get_engine()


def _upload(eng, X):
    """The poison matrix, then X: the rows behind X on the device hold 2^20."""
    eng.null_local_discard()
    eng.upload_x(ed.poison(*X.shape))
    eng.upload_x(X)


def _check_gram(eng, X, what):
    want = X.T @ X
    assert np.abs(want).max() < ed.LIMIT
    _upload(eng, X)
    G = eng.gram()
    np.testing.assert_array_equal(G, G.T, err_msg=what + ': symmetry')
    np.testing.assert_array_equal(G, want, err_msg=what)


@pytest.mark.parametrize('N,n,blk_small,kernel,cap,slab,slabs,passes', ed.GRAM_CASES,
                         ids=['%d-%s%s' % (c[0], c[3], '' if c[2] else '-noblk') for c in ed.GRAM_CASES])
def test_gram_where_a_workgroup_walks_several_slabs(eng, monkeypatch, N, n, blk_small, kernel, cap, slab, slabs, passes):
    """Zero tolerance: G equals the integer X^T X and its own transpose.  Workgroups 0 ... 5 walk three slabs (two in the
    single-buffer kernel): the prefetch under the MFMAs, the store into the other buffer, the buffer swap and a ragged
    `lim` on a slab that is not the first; the rows behind X hold 2^20."""
    monkeypatch.setenv('CNA_GRAM_BLK_SMALL', str(blk_small))
    p = ed.gram_plan(n, N, bool(blk_small))
    assert (p['kernel'], p['cap'], p['slab'], p['slabs'], p['passes'], p['last_rows']) == (kernel, cap, slab, slabs, passes, 7)
    assert p['nblocks'] == cap and n == ed.loop_rows(cap, slab, slabs)
    _check_gram(eng, ed.gram_case(N, n), '%s at %d x %d' % (kernel, n, N))


@pytest.mark.parametrize('N,n', ed.GRAM_SMALL)
def test_gram_of_fewer_rows_than_a_slab(eng, N, n):
    """1, 31 and 33 rows: `lim` cuts the first load, a second workgroup holds one row (three of 16-row slabs at
    N = 640), and the rows behind X hold 2^20."""
    p = ed.gram_plan(n, N)
    assert p['nblocks'] == p['nslab'] == (n + p['slab'] - 1) // p['slab'] and p['last_rows'] < p['slab']
    _check_gram(eng, ed.gram_case(N, n), '%s at %d x %d' % (p['kernel'], n, N))


@pytest.mark.parametrize('N,n,kernel,tiles', ed.XB_CASES, ids=['%d-%d-%s' % (c[0], c[1], c[2].replace(' ', '-')) for c in ed.XB_CASES])
def test_project_and_residualise_twice(eng, N, n, kernel, tiles):
    """Zero tolerance: X . W for a square and a five-column W, X <- (X - m) . M^T and X <- X . M2^T in place, against
    the integer products; the row means are exact integers, the last tile is ragged and the rows behind X hold 2^20."""
    from cna_amd._ffi import MAT_X
    p = ed.xb_plan(n, N, N)
    assert (p['kernel'], p['tiles']) == (kernel, tiles)
    assert p['last_rows'] == {1008: 16, 1029: 5, 131155: 3}[n]             # (63 whole tiles are the contrast)
    assert ed.xb_plan(n, N, 5)['kernel'].split('<')[0] == kernel.split('<')[0]
    c = ed.xb_case(N, n)
    X, m = c['X'], c['m']
    Xc = X - m[:, None]
    np.testing.assert_array_equal(X.sum(axis=1), N * m)
    assert ed.xb_bound(X, c['W']) < ed.LIMIT and ed.xb_bound(X, c['W5']) < ed.LIMIT
    assert ed.xb_bound(Xc, c['M'].T, c['M2'].T) < ed.LIMIT
    _upload(eng, X)
    what = '%s at %d x %d' % (kernel, n, N)
    np.testing.assert_array_equal(eng.project(c['W']), X @ c['W'], err_msg=what + ': X . W')
    np.testing.assert_array_equal(eng.project(c['W5']), X @ c['W5'], err_msg=what + ': X . W5')
    np.testing.assert_array_equal(eng.fetch_matrix(MAT_X), X, err_msg=what + ': X after the projections')
    eng.resid_apply(c['M'], center=True)
    once = Xc @ c['M'].T
    np.testing.assert_array_equal(eng.fetch_matrix(MAT_X), once, err_msg=what + ': (X - m) . M^T')
    eng.resid_apply(c['M2'], center=False)
    np.testing.assert_array_equal(eng.fetch_matrix(MAT_X), once @ c['M2'].T, err_msg=what + ': (X - m) . M^T . M2^T')

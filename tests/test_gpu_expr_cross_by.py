"""cna_expr_cross_by and cna_gram_by on the device, the kernels alone with X from upload_x (run with -m gpu on an MI355X).

Exact inputs.  E holds the integers 0..9, about 60 % present; X comes from exact_grid.grid_matrix: multiples of 2^-4 within
+-4.  Every entry of W is then a multiple of 2^-4 below 2^17 (3 000 x 9 x 4 = 108 000) and every entry of Gamma a multiple of
2^-8 below 2^16 (3 000 x 16 = 48 000): exact in float64 in any order, with or without FMA, on the matrix cores and in numpy
alike.  So there is ONE right answer per level and no tolerance: assert_array_equal.

Shapes.  1 003 cells (seven chunks of 144 cells in the dense kernel, ragged batches of the lists); samples 1, 31, 32, 33, 64, 65,
200 -- the 32-sample tile of k_xcb_dense, the 64-sample width of k_xc_sparse, the 16-wide tiles and 64-wide blocks of
k_gram_by -- with 257 and 1024 in one dense and one gene-major form each; genes 1, 70, 130 (a ragged and a second gene block); levels 1, 3, 33 and 65.
The codes are not sorted, hold -1s, an empty level, a one-cell level, a level whose cells all have xrow = -1 and one level
with 90 % of the cells (as far as the number of levels allows); xrow is a permutation of the rows of a shorter X with -1s.

The forms.  cna_expr_cross_by serves the dense forms.  A one-pass kernel for gene-major lists (accumulators in LDS, indexed by
the level of each entry) was measured slower than one cna_expr_cross per level at 1M cells x 100 samples
(profiles/kbench_gene_test_strata.txt) and by the rule set beforehand is not in the library: Engine.expr_cross_by_raw serves csr
and csc by that masked route, the library entry refuses them, and the cases below hold for all four forms through the engine.

Real inputs against np.longdouble: |err| <= 2 (m_l - 1) 2^-52 sum |terms|, the bound of test_gpu_gene_test.py:check_against,
per level, for W, sx, sxx and Gamma at 33 and 200 samples.  A level of one cell has no sum and the bound is 0: there the
result is one correctly rounded product, compared bit for bit with numpy's."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from numpy.testing import assert_array_equal

from exact_grid import grid_matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ['dense-f32', 'dense-f64', 'csr', 'csc']
CELLS = 1003


def _constant(name, files=('expr_cross_by.hip', 'gram_by.hip', 'genes.hip')):
    src = ''.join(open(os.path.join(ROOT, 'cna_amd', 'csrc', f)).read() for f in files)
    m = re.search(r'constexpr (?:int|int64_t) %s = (\d+)(?:ll)?(?: << (\d+))?;' % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


XCB_MIN_CHUNK = _constant('XCB_MIN_CHUNK')
GB_MIN_CHUNK = _constant('GB_MIN_CHUNK')
LIST_CHUNK = 1024                      # entries of a chunk of a gene's list below 16M entries (genes.hip:build_chunks)


def level_counts(N):
    return [1, 3, 33, 65]


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def as_form(E, form):
    if form == 'dense-f32':
        return np.ascontiguousarray(E, dtype=np.float32)
    if form == 'dense-f64':
        return np.ascontiguousarray(E)
    return sp.csr_matrix(E) if form == 'csr' else sp.csc_matrix(E)


def expression(rs, n, g, integer=True):
    E = (rs.randint(0, 10, (n, g)).astype(np.float64) if integer else rs.gamma(2.0, 1.0, (n, g))) * (rs.rand(n, g) < 0.6)
    E[:, 0] = rs.randint(1, 10, n) if integer else 0.5 + rs.gamma(2.0, 1.0, n)       # gene 0: present in every cell
    return E if integer else E.astype(np.float32).astype(np.float64)                # the four forms hold the same values


def make_xrow(rs, n, frac=0.9):
    took = rs.rand(n) < frac
    xrow = np.full(n, -1, dtype=np.int64)
    xrow[took] = rs.permutation(int(took.sum()))
    return xrow, int(took.sum())


def make_codes(rs, n, L, xrow):
    """int32 codes: about 4 % -1; level 0 takes 90 % of the rest.  From the last level down, as far as L allows: a level of
    one cell (with a row in X), a level whose cells all have xrow = -1, an empty level; the levels between share the
    remainder at random.  The order of the cells is random: the codes are not sorted."""
    codes = np.full(n, -1, dtype=np.int32)
    free = rs.permutation(np.flatnonzero(rs.rand(n) >= 0.04))
    if L == 1:
        codes[free] = 0
        return codes
    one = dead = None
    special = []
    if L >= 2:
        one = L - 1
        cell = free[np.flatnonzero(xrow[free] >= 0)[0]]
        codes[cell] = one
        special.append(cell)
    if L >= 3:
        dead = L - 2
        cells = free[np.flatnonzero(xrow[free] < 0)[:5]]
        codes[cells] = dead
        special.extend(cells)
    rest = np.setdiff1d(free, special)
    rest = rs.permutation(rest)
    nbig = int(0.9 * len(rest))
    codes[rest[:nbig]] = 0
    ordinary = np.arange(1, L - 3)                    # L - 3 stays empty
    if len(ordinary):
        codes[rest[nbig:]] = rs.choice(ordinary, len(rest) - nbig)
    return codes


def level_reference(E, X, xrow, codes, L):
    """(W [L, G, N], sx, sxx [L, G], m [L], Gamma [L, N, N]) in float64 numpy, level by level"""
    G, N = E.shape[1], X.shape[1]
    W, sx, sxx = np.zeros((L, G, N)), np.zeros((L, G)), np.zeros((L, G))
    m, Gam = np.zeros(L, dtype=np.int64), np.zeros((L, N, N))
    for l in range(L):
        sel = np.flatnonzero((codes == l) & (xrow >= 0))
        EK, XK = E[sel], X[xrow[sel]]
        W[l], sx[l], sxx[l], m[l], Gam[l] = EK.T @ XK, EK.sum(axis=0), (EK * EK).sum(axis=0), len(sel), XK.T @ XK
    return W, sx, sxx, m, Gam


def exact_case(N, G, L, n=CELLS, seed=0):
    rs = np.random.RandomState(100000 * seed + 1000 * N + 10 * G + L)
    xrow, nx = make_xrow(rs, n)
    X = grid_matrix(rs, nx, N)
    E = expression(rs, n, G)
    codes = make_codes(rs, n, L, xrow)
    return E, X, xrow, codes


def check_exact(eng, form, N, G, L, masked_levels=6, n=CELLS):
    E, X, xrow, codes = exact_case(N, G, L, n=n)
    want = level_reference(E, X, xrow, codes, L)
    eng.upload_x(X)
    eng.ensure_expression(as_form(E, form))
    got = eng.expr_cross_by_raw(xrow, codes, L)
    for name, a, b in zip(('W', 'sx', 'sxx', 'm'), got, want[:4]):
        assert_array_equal(a, b, err_msg='%s %s N=%d G=%d L=%d' % (name, form, N, G, L))
    again = eng.expr_cross_by_raw(xrow, codes, L)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    # the parent's route, level by level: expr_cross with xrow masked to one level; and all levels together
    pick = sorted(set([0, 1, L // 2, L - 3, L - 2, L - 1]) & set(range(L)))[:masked_levels]
    for l in pick:
        W1, _, sx1, sxx1, m1 = eng.expr_cross(xrow=np.where(codes == l, xrow, -1))
        assert W1.tobytes() == got[0][l].tobytes() and sx1.tobytes() == got[1][l].tobytes(), (form, N, G, L, l)
        assert sxx1.tobytes() == got[2][l].tobytes() and m1 == got[3][l]
    Wall, _, sxa, sxxa, ma = eng.expr_cross(xrow=np.where(codes >= 0, xrow, -1))
    assert_array_equal(got[0].sum(axis=0), Wall)
    assert_array_equal(got[1].sum(axis=0), sxa)
    assert_array_equal(got[2].sum(axis=0), sxxa)
    assert got[3].sum() == ma
    return got


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N', [1, 31, 32, 33, 64, 65, 200])
def test_cross_by_exact_inputs(eng, N, form):
    shapes = [(G, L) for G in (1, 70, 130) for L in (1, 3, 33)] + [(70, L) for L in level_counts(N)[3:]]
    for G, L in shapes:
        check_exact(eng, form, N, G, L, masked_levels=3 if L > 33 else 6)


@pytest.mark.parametrize('form,N', [('csr', 257), ('dense-f64', 257), ('dense-f32', 1024), ('csc', 1024)])
def test_cross_by_exact_inputs_wide(eng, form, N):
    for L in level_counts(N):
        check_exact(eng, form, N, 70, L, masked_levels=3)


def test_cross_by_same_bits_from_csr_and_csc(eng):
    for N, L in ((65, 33), (200, 41)):
        a = check_exact(eng, 'csr', N, 70, L, masked_levels=1)
        b = check_exact(eng, 'csc', N, 70, L, masked_levels=1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('N', [1, 31, 32, 33, 64, 65, 200, 257, 1024])
def test_gram_by_exact_inputs(eng, N):
    for L in level_counts(N):
        E, X, xrow, codes = exact_case(N, 1, L)
        want = level_reference(E, X, xrow, codes, L)
        eng.upload_x(X)
        Gam, m = eng.gram_by(xrow, codes, L)
        assert_array_equal(m, want[3])
        assert_array_equal(Gam, want[4], err_msg='N=%d L=%d' % (N, L))
        again, _ = eng.gram_by(xrow, codes, L)
        assert again.tobytes() == Gam.tobytes()
        # all levels together: cna_gram of the rows of X of the coded cells
        rows = xrow[(codes >= 0) & (xrow >= 0)]
        eng.upload_x(X[rows])
        assert_array_equal(Gam.sum(axis=0), eng.gram())


# ------------------------------------------------------------------ real inputs
def _bound_ratio(got, want, mag, m):
    u = 2.0 * max(m - 1, 0) * 2.0 ** -52
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bound = (u * mag).astype(np.float64)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


@pytest.mark.parametrize('N', [33, 200])
def test_real_inputs_against_longdouble(eng, N):
    G, L, n = 70, 7, CELLS
    rs = np.random.RandomState(N)
    xrow, nx = make_xrow(rs, n)
    X = rs.randn(nx, N) * (1.0 + rs.rand(N)) + rs.randn(N)
    E = expression(rs, n, G, integer=False)
    codes = make_codes(rs, n, L, xrow)
    eng.upload_x(X)
    Gam, mg = eng.gram_by(xrow, codes, L)
    outs = {}
    for form in FORMS:
        Ef = as_form(E, form)
        assert np.array_equal(np.asarray(Ef.todense()) if sp.issparse(Ef) else Ef.astype(np.float64), E)
        eng.ensure_expression(Ef)
        outs[form] = eng.expr_cross_by_raw(xrow, codes, L)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs['csr'], outs['csc']))
    worst = {}
    for l in range(L):
        sel = np.flatnonzero((codes == l) & (xrow >= 0))
        EK, XK = E[sel].astype(np.longdouble), X[xrow[sel]].astype(np.longdouble)
        m = len(sel)
        assert mg[l] == m
        if m <= 1:
            # no sum at all: the bound is 0, and what is right is the one correctly rounded product (or 0), bit for bit
            E1, X1 = E[sel], X[xrow[sel]]
            one = (E1.T * X1 if m else np.zeros((G, N)), E1.sum(axis=0), (E1 * E1).sum(axis=0))
            for form in FORMS:
                assert outs[form][3][l] == m
                for a, b in zip(outs[form][:3], one):
                    assert_array_equal(a[l], b)
            assert_array_equal(Gam[l], X1.T * X1 if m else np.zeros((N, N)))
            continue
        refs = [('W', EK.T @ XK, np.abs(EK).T @ np.abs(XK)), ('sx', EK.sum(axis=0), np.abs(EK).sum(axis=0)),
                ('sxx', (EK * EK).sum(axis=0), (EK * EK).sum(axis=0))]
        for form in FORMS:
            assert outs[form][3][l] == m
            for j, (name, want, mag) in enumerate(refs):
                k = '%s %s' % (form, name)
                worst[k] = max(worst.get(k, 0.0), _bound_ratio(outs[form][j][l], want, mag, m))
        worst['Gamma'] = max(worst.get('Gamma', 0.0), _bound_ratio(Gam[l], XK.T @ XK, np.abs(XK).T @ np.abs(XK), m))
    for k in sorted(worst):
        print('N=%d %s: max |err| / bound = %.3e' % (N, k, worst[k]))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------ the fold across chunks
def test_more_than_two_chunks_per_level(eng):
    """3 000 cells, level 0 with 90 % of them: more than two chunks of the dense kernel's cell list (XCB_MIN_CHUNK cells at
    least, the slab rule of cna_expr_cross above that), more than two chunks of GB_MIN_CHUNK rows in k_gram_by, and gene 0,
    present in every cell, with more than two list chunks of LIST_CHUNK entries."""
    n, N, G, L = 3000, 33, 5, 3
    E, X, xrow, codes = exact_case(N, G, L, n=n, seed=1)
    big = int(((codes == 0) & (xrow >= 0)).sum())
    dense_chunk = max(XCB_MIN_CHUNK, math.ceil(n / (n // XCB_MIN_CHUNK)))
    assert big > 2 * dense_chunk and big > 2 * GB_MIN_CHUNK and (E[:, 0] != 0).sum() > 2 * LIST_CHUNK
    assert ((codes == 0) & (E[:, 0] != 0))[2 * LIST_CHUNK:].any()
    want = level_reference(E, X, xrow, codes, L)
    for form in FORMS:
        got = check_exact_given(eng, form, E, X, xrow, codes, L, want)
        assert got[3][0] == big
    Gam, m = eng.gram_by(xrow, codes, L)
    assert_array_equal(Gam, want[4])
    assert m[0] == big


def check_exact_given(eng, form, E, X, xrow, codes, L, want, bin0=0, nb=None):
    nb = L - bin0 if nb is None else nb
    eng.upload_x(X)
    eng.ensure_expression(as_form(E, form))
    got = eng.expr_cross_by_raw(xrow, codes, L, bin0, nb)
    for name, a, b in zip(('W', 'sx', 'sxx', 'm'), got, want[:4]):
        assert_array_equal(a, b[bin0:bin0 + nb], err_msg='%s %s' % (name, form))
    return got


@pytest.mark.parametrize('form', FORMS)
def test_a_second_level_group(eng, form):
    """bin0 > 0 with nb < n_bins"""
    for N, L, bin0, nb in ((33, 33, 7, 9), (200, 60, 11, 43)):
        E, X, xrow, codes = exact_case(N, 70, L, seed=2)
        want = level_reference(E, X, xrow, codes, L)
        check_exact_given(eng, form, E, X, xrow, codes, L, want, bin0, nb)
        check_exact_given(eng, form, E, X, xrow, codes, L, want, L - 1, 1)


def test_engine_level_groups_match_the_single_call(eng, monkeypatch):
    """Engine.expr_cross_by in groups of levels (a result that does not fit its host budget) against the single call, and
    `bins`."""
    N, G, L = 65, 70, 33
    E, X, xrow, codes = exact_case(N, G, L, seed=3)
    want = level_reference(E, X, xrow, codes, L)
    eng.upload_x(X)
    eng.ensure_expression(as_form(E, 'csr'))
    whole = eng.expr_cross_by(codes, L, xrow=xrow)
    rho = np.stack([X[xrow[(codes == l) & (xrow >= 0)]].sum(axis=0) for l in range(L)])
    for a, b in zip(whole, (want[0], rho, want[1], want[2], want[3], want[4])):
        assert_array_equal(a, b)
    monkeypatch.setattr(type(eng), 'CROSS_BY_HOST_BYTES', 8 * G * N * 5)       # five levels of W, two of Gamma per group
    grouped = eng.expr_cross_by(codes, L, xrow=xrow)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, grouped))
    some = eng.expr_cross_by(codes, L, bins=[30, 2, 0], xrow=xrow)
    assert all(a.tobytes() == b[[30, 2, 0]].tobytes() for a, b in zip(some, whole))


# ------------------------------------------------------------------ NaN and Inf stay where they are
@pytest.mark.parametrize('form', FORMS)
def test_nan_and_inf_touch_only_their_own_gene_and_level(eng, form):
    N, G, L = 33, 70, 7
    E, X, xrow, codes = exact_case(N, G, L, seed=4)
    eng.upload_x(X)

    def run(M):
        eng.ensure_expression(as_form(M, form))
        return eng.expr_cross_by_raw(xrow, codes, L)
    clean = run(E)
    part = np.flatnonzero((codes >= 0) & (xrow >= 0))
    lvl0, lvl2 = part[codes[part] == 0], part[codes[part] == 2]
    hit = {(0, 0): (lvl0[len(lvl0) // 2], np.nan), (0, 9): (lvl0[0], np.inf), (2, 64): (lvl2[-1], -np.inf)}
    D = E.copy()
    for (l, g), (cell, v) in hit.items():
        D[cell, g] = v
    got = run(D)
    bad = np.zeros((L, G), dtype=bool)
    for l, g in hit:
        bad[l, g] = True
    assert_array_equal(got[3], clean[3])
    for a, b in zip(got[:3], clean[:3]):
        assert not np.isfinite(a[bad]).any()
        assert a[~bad].tobytes() == b[~bad].tobytes()
    assert np.isnan(got[1][0, 0]) and got[1][0, 9] == np.inf and got[1][2, 64] == -np.inf and got[2][2, 64] == np.inf
    # in cells that take part in no level: never read into a sum
    out = np.flatnonzero((codes < 0) | (xrow < 0))
    D = E.copy()
    D[out[0], 0], D[out[len(out) // 2], 9], D[out[-1], 64] = np.nan, np.inf, -np.inf
    got = run(D)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, clean))


# ------------------------------------------------------------------ refusals
def _raw(e, xrow, codes, n_bins, G, N, bin0=0, nb=None):
    """(rc of cna_expr_cross_by, rc of cna_gram_by, whether every output of the one / of the other still holds its sentinel)"""
    from cna_amd._ffi import ptr
    nb = n_bins if nb is None else nb
    k = max(min(nb, 2048), 1)
    xrow = np.ascontiguousarray(xrow, dtype=np.int64)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    bufs = [np.full((k, G, N), 7.5), np.full((k, G), 7.5), np.full((k, G), 7.5), np.full(k, -5, dtype=np.int64)]
    rc1 = e.lib.cna_expr_cross_by(e.h, ptr(xrow), ptr(codes), len(xrow), n_bins, bin0, nb, *[ptr(b) for b in bufs])
    kg = n_bins if 1 <= n_bins <= 1024 else 1
    gb = [np.full((kg, N, N), 7.5), np.full(kg, -5, dtype=np.int64)]
    rc2 = e.lib.cna_gram_by(e.h, ptr(xrow), ptr(codes), len(xrow), n_bins, ptr(gb[0]), ptr(gb[1]))
    cross_untouched = all((b == 7.5).all() for b in bufs[:3]) and (bufs[3] == -5).all()
    gram_untouched = (gb[0] == 7.5).all() and (gb[1] == -5).all()
    return rc1, rc2, cross_untouched, gram_untouched


def test_refusals_leave_the_outputs_untouched(eng):
    from cna_amd._ffi import CnaHipError
    from cna_amd.engine import Engine
    N, G, L = 33, 5, 4
    E, X, xrow, codes = exact_case(N, G, L, seed=5)
    eng.upload_x(X)
    eng.ensure_expression(as_form(E, 'dense-f32'))
    nx = X.shape[0]
    named = np.flatnonzero(xrow >= 0)
    cases = {'a code too large': (xrow, np.where(np.arange(CELLS) == 17, L, codes), 'a code lies outside'),
             'a code below -1': (xrow, np.where(np.arange(CELLS) == 900, -2, codes), 'a code lies outside'),
             'an xrow too large': (np.where(np.arange(CELLS) == named[3], nx, xrow), codes, 'an xrow lies outside'),
             'an xrow below -1': (np.where(np.arange(CELLS) == 5, -2, xrow), codes, 'an xrow lies outside'),
             'an xrow twice': (np.where(np.arange(CELLS) == named[7], xrow[named[8]], xrow), codes, 'two cells name the same row')}
    for name, (xr, cd, msg) in cases.items():
        rc1, rc2, u1, u2 = _raw(eng, xr, cd, L, G, N)
        assert (rc1, rc2) == (-1, -1) and u1 and u2, name                   # CNA_EINVAL
        assert msg in eng.lib.cna_last_error().decode(), name
    for n_bins in (0, 1025):
        rc1, rc2, u1, u2 = _raw(eng, xrow, np.minimum(codes, 0), n_bins, G, N)
        assert (rc1, rc2) == (-1, -1) and u1 and u2, n_bins
        assert '1 <= n_bins <= 1024' in eng.lib.cna_last_error().decode()
    for bin0, nb in ((-1, 2), (3, 2), (0, 0), (4, 1)):
        rc1, _, u1, _ = _raw(eng, xrow, codes, L, G, N, bin0, nb)
        assert rc1 == -1 and u1, (bin0, nb)
    rc1, rc2, u1, u2 = _raw(eng, xrow[:-1], codes[:-1], L, G, N)            # another length than the matrix' cells
    assert rc1 == -1 and u1 and rc2 == 0 and not u2
    # the inputs themselves pass
    rc1, rc2, u1, u2 = _raw(eng, xrow, codes, L, G, N)
    assert (rc1, rc2) == (0, 0) and not u1 and not u2
    # gene-major lists: refused by the library entry (the engine serves them by the masked route, checking the codes itself)
    eng.ensure_expression(as_form(E, 'csr'))
    rc1, rc2, u1, u2 = _raw(eng, xrow, codes, L, G, N)
    assert rc1 == -4 and u1 and rc2 == 0 and not u2 and 'gene-major' in eng.lib.cna_last_error().decode()
    with pytest.raises(CnaHipError, match='a code lies outside'):           # the engine's own checks: the library's error type
        eng.expr_cross_by_raw(xrow, np.where(np.arange(CELLS) == 17, L, codes), L)
    with pytest.raises(CnaHipError, match='n_bins'):
        eng.expr_cross_by_raw(xrow, codes, 1025)
    eng.ensure_expression(as_form(E, 'dense-f32'))
    with pytest.raises(CnaHipError, match='a code lies outside'):           # ... as the dense form raises it
        eng.expr_cross_by_raw(xrow, np.where(np.arange(CELLS) == 17, L, codes), L)
    # no expression matrix resident: the Gram matrices need none
    eng.drop_expression()
    rc1, rc2, u1, u2 = _raw(eng, xrow, codes, L, G, N)
    assert rc1 == -4 and u1 and rc2 == 0 and not u2                         # CNA_ESTATE, nothing written
    assert 'no expression matrix' in eng.lib.cna_last_error().decode()
    # X void
    other = Engine()
    try:
        other.ensure_expression(as_form(E, 'dense-f32'))
        rc1, rc2, u1, u2 = _raw(other, xrow, codes, L, G, N)
        assert (rc1, rc2) == (-4, -4) and u1 and u2
        assert 'X not available' in other.lib.cna_last_error().decode()
    finally:
        other.close()


def test_gram_by_refuses_more_than_one_gib(eng):
    from cna_amd._ffi import ptr
    N = 1024
    rs = np.random.RandomState(0)
    X = grid_matrix(rs, 40, N)
    eng.upload_x(X)
    xrow = np.arange(40, dtype=np.int64)
    codes = np.zeros(40, dtype=np.int32)
    n_bins = (1 << 30) // (8 * N * N) + 1                                   # 129 levels x 8 MiB
    out, m = np.full((1, N, N), 7.5), np.full(n_bins, -5, dtype=np.int64)
    rc = eng.lib.cna_gram_by(eng.h, ptr(xrow), ptr(codes), 40, n_bins, ptr(out), ptr(m))
    assert rc == -1 and 'exceed 1 GiB' in eng.lib.cna_last_error().decode()
    assert (out == 7.5).all() and (m == -5).all()
    Gam, m = eng.gram_by(xrow, codes, n_bins - 1)                           # ... and 128 levels pass
    assert_array_equal(Gam[0], X.T @ X)
    assert not Gam[1:].any() and m[0] == 40 and not m[1:].any()

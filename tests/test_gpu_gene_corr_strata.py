"""cna.tl.gene_corr_strata on the device (run with -m gpu on an MI355X).

Bounds, the project's own: 1e-10 absolute on r and on the within-level correlation against the float64 numpy restatement of
tests/test_gene_corr_strata_host.py, with equal NaN patterns; 1e-5 against the reference's own line, level by level.  Every
parity input is benign for the raw-moment variance (test_gpu_parity_inputs_are_benign_for_raw_moments checks
sum x^2 / sum (x - mean)^2 <= 100 per (key, level, gene) on the CPU), so the first bound tests the kernels and not the formula.
The observed maxima are written to the file CNA_GENE_STRATA_PARITY_OUT names, when it is set
(profiles/r12_gene_corr_strata_parity.txt is such a run's output)."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_gene_corr_host import restated_gene_corr, dense_expression, sparse_expression, keys_for
from test_gene_corr_strata_host import (restated_gene_corr_strata, levels_for, with_benign_pair, parity_input, PARITY_CASES,
                                        N_ODD)

pytestmark = pytest.mark.gpu

REF_TOL = 1e-5      # floats against the reference
F64_TOL = 1e-10     # GPU against an f64 restatement
_seen = {}


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()
    if os.environ.get('CNA_GENE_STRATA_PARITY_OUT') and _seen:
        with open(os.environ['CNA_GENE_STRATA_PARITY_OUT'], 'w') as f:
            f.write('max |gpu - restated| per case of tests/test_gpu_gene_corr_strata.py, r and within (bound %g; reference line: %g)\n'
                    % (F64_TOL, REF_TOL))
            for k in sorted(_seen):
                f.write('%-66s %.3e\n' % (k, _seen[k]))
            f.write('%-66s %.3e\n' % ('maximum', max(_seen.values())))


def _check(name, got, want, tol=F64_TOL):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=name)
    err = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    _seen[name] = max(err, _seen.get(name, 0.0))
    print('%s: max |d| = %.3e (bound %g)' % (name, err, tol))
    assert err <= tol, (name, err)


def _run(eng, X, V, codes, L, want_within=True):
    eng.ensure_expression(X)
    return eng.gene_corr_by(V, codes, L, want_within=want_within)


def _parity(eng, name, X, V, codes, L, want):
    r, within, n = _run(eng, X, V, codes, L)
    np.testing.assert_array_equal(n, want[2], err_msg=name)
    _check(name + ' r', r, want[0])
    _check(name + ' within', within, want[1])
    return r, within


@functools.lru_cache(maxsize=None)
def _sparse_reference(case):
    """One restatement per case for its four gene-major uploads: their values are small integers, the same in f32 and f64."""
    X, V, codes = parity_input('sparse', *case)
    return restated_gene_corr_strata(X, V, codes, case[2])


# ------------------------------------------------------------------ 1. against the restatement
# 3001 x 70 with (levels, keys, masks): the kernels are instantiated for Q = 1, 2, 4, 8, 16 key slots and for one shared mask
# or one per key -- (1, 1, none) Q = 1 shared and the one-level path of the gene-major kernel, (2, 2, equal) Q = 2 full shared,
# (17, 3, differ) Q = 4 padded, (64, 5, differ) Q = 8 padded, (16, 16, differ) Q = 16 full, (33, 1, equal) a level count that is
# a multiple of neither 16 nor 64; from four levels on the last two levels have two cells and one cell
SMALL = [c for c in PARITY_CASES if c[0] == N_ODD]


@pytest.mark.parametrize('case', SMALL, ids=lambda c: 'L%d-q%d-%s' % c[2:])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_dense_against_restatement(eng, dtype, case):
    X, V, codes = parity_input('dense', *case, dtype=dtype)
    _parity(eng, 'dense %s L=%d q=%d masks=%s' % ((np.dtype(dtype).name,) + case[2:]), X, V, codes, case[2],
            restated_gene_corr_strata(X, V, codes, case[2]))
    assert eng.expression_shape()['format'] == 'dense'


@pytest.mark.parametrize('case', SMALL, ids=lambda c: 'L%d-q%d-%s' % c[2:])
@pytest.mark.parametrize('fmt,index_dtype,dtype', [('csr', np.int32, np.float32), ('csr', np.int64, np.float64),
                                                   ('csc', np.int32, np.float64), ('csc', np.int64, np.float32)])
def test_sparse_against_restatement(eng, fmt, index_dtype, dtype, case):
    X, V, codes = parity_input('sparse', *case, dtype=dtype, fmt=fmt, index_dtype=index_dtype)
    assert X.format == fmt and X.indices.dtype == index_dtype and X.dtype == dtype
    assert X.getnnz(axis=0)[0] >= N_ODD - 2 and X.getnnz(axis=0)[1] <= 5                   # the skew genes stay
    _parity(eng, '%s %s %s L=%d q=%d masks=%s' % ((fmt, np.dtype(index_dtype).name, np.dtype(dtype).name) + case[2:]), X, V,
            codes, case[2], _sparse_reference(case))
    assert eng.expression_shape()['format'] == 'gene-major'


@pytest.mark.parametrize('kind', ['dense', 'csr'])
def test_many_levels(eng, kind):
    """20011 x 70 in 256 levels, two keys with their own masks."""
    case = (20011, 70, 256, 2, 'differ')
    X, V, codes = parity_input('dense' if kind == 'dense' else 'sparse', *case, dtype=np.float32)
    want = restated_gene_corr_strata(X, V, codes, 256) if kind == 'dense' else _sparse_reference(case)
    _parity(eng, '%s f32 20011 x 70 L=256 q=2' % kind, X, V, codes, 256, want)


@pytest.mark.parametrize('kind', ['dense', 'csr'])
def test_the_row_limit_takes_several_passes(eng, kind):
    """80021 x 40 in 1024 levels with four keys of their own masks: q x levels = 4096, the limit.  On the gene-major form a
    level's record has 5 S + Q = 24 fields of 8 bytes and a turn word of 4 (S = Q = 4: the masks differ), so 1024 levels
    would need 200 704 bytes of LDS; k_cb_sparse is launched with 64 KB at most, which holds 334 levels: the lists are read
    in four passes of 256 levels.  On the dense form the 1024 chunks of the cell list (no level reaches 2048 cells) are finished
    in groups of at most q x levels / F + cells / 2048 = 243 chunks (F = 4 S + Q = 20), five launches."""
    case = (80021, 40, 1024, 4, 'differ')
    assert 1024 * (8 * (5 * 4 + 4) + 4) > 3 * 65536
    X, V, codes = parity_input('dense' if kind == 'dense' else 'sparse', *case, dtype=np.float32)
    want = restated_gene_corr_strata(X, V, codes, 1024) if kind == 'dense' else _sparse_reference(case)
    r, within = _parity(eng, '%s f32 80021 x 40 L=1024 q=4' % kind, X, V, codes, 1024, want)
    assert np.isnan(r[:, 1023]).all()                                             # the level of one cell
    assert np.isfinite(r[:, 300:1000, 2:]).mean() > 0.8                           # levels of the later passes are filled in


def test_more_chunks_than_levels_and_more_than_one_gene_block(eng):
    """40013 x 300 in 7 levels: five levels of ~7800 cells, four chunks of the cell list each, 300 genes in two gene blocks."""
    case = (40013, 300, 7, 2, 'differ')
    X, V, codes = parity_input('dense', *case, dtype=np.float32)
    assert np.bincount(codes[codes >= 0])[:5].min() > 3 * 2048
    _parity(eng, 'dense f32 40013 x 300 L=7 q=2', X, V, codes, 7, restated_gene_corr_strata(X, V, codes, 7))


# ------------------------------------------------------------------ 2. exactness of the constants
def test_constants_are_decided_exactly(eng):
    n, L = N_ODD, 6
    codes = levels_for(n, L, seed=41)
    X = with_benign_pair(dense_expression(n, 20, seed=9), codes, L)
    V = keys_for(n, 3, seed=9, masks='differ')
    X[:, 3] = 2.5                                   # constant everywhere: raw moments alone would give garbage, not NaN
    X[codes != 2, 4] = 1e-3                         # constant in every level but one
    X[codes == 1, 5] = 7.0                          # constant in one level
    X[codes == 3, 6] = 0.0                          # an all-zero gene inside one level (no entries in the lists)
    V[1, codes == 2] = 0.75                         # a key that is constant in one level
    V[2, codes == 0] = np.nan                       # a key without any cell in one level
    want = restated_gene_corr_strata(X, V, codes, L)
    r, within = want[0], want[1]
    assert np.isnan(r[:, :, 3]).all() and np.isnan(within[:, 3]).all()
    assert np.isnan(r[0, [0, 1, 3, 4, 5], 4]).all() and np.isfinite(r[0, 2, 4]) and np.isfinite(within[0, 4])
    assert np.isnan(r[1, :, 4]).all()                                        # ... and there key 1 is constant
    assert np.isnan(r[:, 1, 5]).all() and np.isfinite(within[:, 5]).all() and np.isnan(r[1, 2]).all() and np.isnan(r[2, 0]).all()
    assert want[2][2, 0] == 0
    _parity(eng, 'constants dense', X, V, codes, L, want)
    # gene 4 varies in level 2 alone and key 1 is constant there: no level adds to their covariance, not even rounding residue
    assert within[1, 4] == 0.0 and _run(eng, X, V, codes, L)[1][1, 4] == 0.0
    for fmt in ('csr', 'csc'):
        got = _parity(eng, 'constants %s' % fmt, sp.csr_matrix(X).asformat(fmt), V, codes, L, want)
        assert got[1][1, 4] == 0.0


# ------------------------------------------------------------------ 3. the reference's line, level by level
def test_the_demo_line_inside_every_cluster(eng):
    import cna_amd as cna
    from cna_amd import synth
    d, samplem = synth.make_demo_like(keep_expression=True)
    cna.tl.association(d, samplem['case'].astype(float), 'id', key_added='coef', Nnull=200, seed=0, engine=eng)
    G = d.X.shape[1]
    lo, hi = d.X[:, :G // 2].mean(axis=1), d.X[:, G // 2:].mean(axis=1)
    pop = np.where(hi > lo, 'B', np.where(lo > 1.2, 'C', 'A'))               # the three populations, as a clustering finds them
    d.obs['leiden'] = [p + str(i % 4) for p, i in zip(pop, np.random.RandomState(1).permutation(len(pop)))]
    frame, within = cna.tl.gene_corr_strata(d, 'leiden', return_within=True, engine=eng)
    levels = list(pd.unique(d.obs['leiden']))
    assert len(levels) == 12 and list(frame.columns) == levels and frame.index.equals(d.var_names)
    v = d.obs['coef'].values.astype(np.float64)
    assert np.isfinite(v).sum() > 0.9 * len(v)
    for name in levels:
        w = (d.obs['leiden'].values == name) & np.isfinite(v)
        with np.errstate(all='ignore'):
            want = np.corrcoef(v[w], d.X[w], rowvar=False)[0, 1:]
        _check('demo line, level %s' % name, frame[name].values, want, REF_TOL)
    codes = pd.factorize(d.obs['leiden'])[0].astype(np.int32)
    want = restated_gene_corr_strata(d.X, v, codes, 12)
    _check('demo-like vs restatement r', frame.values.T, want[0][0])
    _check('demo-like vs restatement within', within['coef'].values, want[1][0])
    # what the call is for: the global line sees the populations, the adjusted one does not
    glob = cna.tl.gene_corr(d, 'coef', engine=eng)['coef'].values
    assert np.nanmax(np.abs(glob)) > 0.2 and np.isfinite(within['coef'].values).all()


# ------------------------------------------------------------------ 4. agreement with the existing kernels
@pytest.mark.parametrize('kind', ['dense', 'csr'])
def test_agrees_with_gene_corr_on_masked_keys(eng, kind):
    """What the parent commit could do: the key masked to one level, sixteen such columns per cna_gene_corr call."""
    n, L = N_ODD, 17
    X, V, codes = parity_input('dense' if kind == 'dense' else 'sparse', n, 70, L, 1, 'equal', dtype=np.float32)
    r, within, cnt = _run(eng, X, V, codes, L)
    masked = np.where(codes[None, :] == np.arange(L)[:, None], V[0][None, :], np.nan)
    emu = np.concatenate([eng.gene_corr(masked[k:k + 16]) for k in range(0, L, 16)])
    _check('emulation through gene_corr %s' % kind, r[0], emu)
    np.testing.assert_array_equal(cnt[0], np.bincount(codes[(codes >= 0) & np.isfinite(V[0])], minlength=L))


@pytest.mark.parametrize('kind', ['dense', 'csr'])
def test_two_calls_give_the_same_bits(eng, kind):
    case = (20011, 70, 33, 5, 'differ')
    X, V, codes = parity_input('dense' if kind == 'dense' else 'sparse', *case, dtype=np.float32)
    a = _run(eng, X, V, codes, 33)
    b = eng.gene_corr_by(V, codes, 33)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    c = eng.gene_corr_by(V, codes, 33, want_within=False)
    assert c[1] is None
    np.testing.assert_array_equal(a[0], c[0])


# ------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize('kind', ['dense', 'csr'])
def test_bad_codes_are_refused_and_harm_nothing(eng, kind):
    from cna_amd._ffi import CnaHipError
    n, L = N_ODD, 17
    X, V, codes = parity_input('dense' if kind == 'dense' else 'sparse', n, 70, L, 3, 'differ')
    want = restated_gene_corr_strata(X, V, codes, L)
    _parity(eng, 'before the refusals %s' % kind, X, V, codes, L, want)
    ups = eng.expression_shape()['uploads']
    for bad_value in (L, -2):
        bad = codes.copy()
        bad[n // 2] = bad_value
        with pytest.raises(CnaHipError, match='outside'):
            eng.gene_corr_by(V, bad, L)
    with pytest.raises(CnaHipError):
        eng.gene_corr_by(V, codes, 1025)
    with pytest.raises(CnaHipError, match='4096'):
        eng.gene_corr_by(np.tile(V, (2, 1))[:5], np.zeros(n, dtype=np.int32), 1000)
    with pytest.raises(ValueError):
        eng.gene_corr_by(V[:, :-1], codes[:-1], L)
    assert eng.expression_shape()['uploads'] == ups and eng.expression_shape()['n_cells'] == n
    r, within, cnt = eng.gene_corr_by(V, codes, L)
    _check('after the refusals %s r' % kind, r, want[0])
    _check('after the refusals %s within' % kind, within, want[1])
    _check('gene_corr after the refusals %s' % kind, eng.gene_corr(V), restated_gene_corr(X, V))


def test_no_resident_matrix_is_refused(eng):
    from cna_amd._ffi import CnaHipError
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    with pytest.raises(CnaHipError, match='no expression matrix'):
        eng.gene_corr_by(np.zeros((1, 10)), np.zeros(10, dtype=np.int32), 1)
    X, V, codes = parity_input('dense', N_ODD, 70, 17, 3, 'differ', dtype=np.float32)
    _run(eng, X, V, codes, 17)
    assert eng.device_bytes() > base
    eng.drop_expression()                           # the work buffers go with the matrix
    assert eng.device_bytes() == base

"""cna.tl.gene_rank_corr on the CPU: the numpy / scipy restatement of cna_gene_rank_corr (what the GPU tests compare the device
with, integer for integer), its check against scipy.stats.spearmanr on the GPU tests' own inputs, the public call against an
engine double (GeneEngine of test_gene_corr_host.py with `gene_rank_corr` backed by the restatement), and the proofs, without
a device, that the GPU inputs reach what they are meant to reach: three sort chunks per long gene and per key, two tiles of
genes and one tile per key under the small budget (recomputed for the 4-byte payload), tie runs of a gene and of a key that
end on a cut of the kernels' unit and that span two, and a sum that passes 64 bits.  The constants of csrc/rank_sort.h and
csrc/expr_rankcorr.hip are read from the source."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import scipy.stats

from test_gene_corr_host import GeneEngine, _frame
from test_gene_markers_host import (FORMS, N_CORE, ROOT, RUN_ON_CUT, RUN_OVER_CUTS, SMALL_WORK_BYTES, _dense, core_codes,
                                    core_input, core_values, markers_input, ranksum_constant, ranksum_source, sort_chunks)

RHO_TOL = 1e-10         # the project's figure for z in test_gene_markers_host.py
WIDE_CELLS = 3100000    # the GPU tests' wide case
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------ the restatement
def _centred(col, m):
    """2 x midrank - (m + 1) as int64: |.| <= m - 1, sums to 0"""
    return np.rint(2.0 * scipy.stats.rankdata(col, method='average')).astype(np.int64) - (m + 1)


def _tie_term(col):
    return float(sum(int(t) ** 3 - int(t) for t in np.unique(col, return_counts=True)[1]))


def restated_rank_corr(X, V):
    """(S object[q, G] of Python ints, tie_gene float64[G], tie_key float64[q], m, nan bool[G]) of cna_gene_rank_corr: scipy's
    midranks of the rows where every key is finite, doubled and centred; S = sum a b in exact integers; the tie terms from
    np.unique's counts.  A gene with a NaN in a kept cell is flagged and its numbers are 0 (the device leaves them
    unspecified: callers compare the other genes)."""
    Xd = _dense(X)
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    kept = np.isfinite(V).all(axis=0)
    m = int(kept.sum())
    q, G = V.shape[0], Xd.shape[1]
    S = np.zeros((q, G), dtype=object)
    S[...] = 0
    tie_gene, tie_key, nan = np.zeros(G), np.zeros(q), np.zeros(G, dtype=bool)
    b = [_centred(V[k, kept], m) for k in range(q)]
    for k in range(q):
        tie_key[k] = _tie_term(V[k, kept] + 0.0)               # -0.0 + 0.0 = +0.0: one value
    fits = (m ** 3 - m) // 3 < 2 ** 63
    for g in range(G):
        col = Xd[kept, g].astype(np.float64)                   # exact from float32: the order and the ties of the stored type
        if np.isnan(col).any():
            nan[g] = True
            continue
        if m == 0:
            continue
        a = _centred(col, m)
        tie_gene[g] = _tie_term(col + 0.0)
        for k in range(q):
            S[k, g] = int(np.dot(a, b[k])) if fits else int(np.dot(a.astype(object), b[k].astype(object)))
    return S, tie_gene, tie_key, m, nan


def limbs(S):
    """Python ints -> (low 64 bits uint64, the limb above int64) of their 128-bit two's complement"""
    lo = np.array([[int(s) & MASK64 for s in row] for row in S], dtype=np.uint64).reshape(S.shape)
    hi = np.array([[int(s) >> 64 for s in row] for row in S], dtype=np.int64).reshape(S.shape)
    return lo, hi


def as_engine(restated):
    """the restatement in the shape Engine.gene_rank_corr returns"""
    S, tie_gene, tie_key, m, nan = restated
    lo, hi = limbs(S)
    return lo, hi, tie_gene, tie_key, m, nan


# ------------------------------------------------------------------ the GPU tests' inputs
KEY_RUN_ON_CUT, KEY_RUN_OVER_CUTS = 256, 700     # key 1: kept cells with its smallest value, then with the next one


@functools.lru_cache(maxsize=None)
def core_keys(q=3):
    """float64 [q, 3001] for the nine core genes: NaN where core_codes() < 0 in every key, five NaNs of its own in key 0 (the
    kept set is the intersection), then
      0: distinct values
      1: heavy ties, -0.0 and +0.0 among them; its smallest value in exactly 256 kept cells, the next one in 700
      2: a strictly increasing transform of gene 1: S = (m^3 - m) / 3, no tie on either side
    q = 1: key 0 alone; q = 16: these three, then ties of every weight and monotone transforms of each other."""
    n = N_CORE
    rs = np.random.RandomState(77)
    codes = core_codes()
    Vg, Sg = core_values()
    V = np.empty((max(q, 3), n))
    V[0] = rs.randn(n)
    own = np.flatnonzero((codes >= 0) & ~Sg[:, 4])             # not among gene 4's stored entries: its runs keep their cuts
    own = own[own > np.flatnonzero(codes >= 0)[8]][[3, 400, 700, 1000, 1300]]
    V[0, own] = [np.nan, np.inf, -np.inf, np.nan, np.nan]      # non-finite of every kind: the cell is left out
    kept = np.flatnonzero((codes >= 0) & np.isfinite(V[0]))
    order = rs.permutation(kept)
    a, b = KEY_RUN_ON_CUT, KEY_RUN_ON_CUT + KEY_RUN_OVER_CUTS
    V[1] = 7.0
    V[1, order[:a]] = -3.0
    V[1, order[a:b]] = -1.0
    V[1, order[b:b + 600:2]] = -0.0
    V[1, order[b + 1:b + 600:2]] = 0.0
    V[1, order[b + 600:b + 1100]] = 1.0
    V[1, order[b + 1100:b + 1103]] = 2.5
    V[2] = Vg[:, 1] ** 3 + 1.0
    for k in range(3, V.shape[0]):
        if k % 3 == 0:
            V[k] = rs.randint(0, 1 << (k // 3), size=n)        # 2, 4, 8, ... distinct values
        elif k % 3 == 1:
            V[k] = -np.exp(V[0] / (1.0 + k))                   # a decreasing transform of key 0
            V[k, own] = 0.0
        else:
            V[k] = rs.standard_cauchy(n) * 10.0 ** rs.randint(-300, 300)   # heavy tails over the whole exponent range
    V[:, codes < 0] = np.nan
    V = np.ascontiguousarray(V[:q])
    V.setflags(write=False)
    return V


def core_kept():
    return np.isfinite(core_keys()).all(axis=0)


@functools.lru_cache(maxsize=None)
def core_rank_reference(form, q=3):
    """One restatement per stored type and key count: the sparse and the dense upload of one type hold the same values."""
    Vg, _ = core_values()
    out = restated_rank_corr(Vg.astype(np.float32 if form.endswith('f32') else np.float64), core_keys(q))
    for a in (out[1], out[2], out[4]):
        a.setflags(write=False)
    return out


def wide_input():
    """(X float32 [3 100 000, 2], key float64, S of gene 0): gene 0 a fixed permutation's distinct values, gene 1 their
    negation, the key an increasing transform of gene 0: S = +-(m^3 - m) / 3 in closed form"""
    m = WIDE_CELLS
    x = np.random.RandomState(31).permutation(m).astype(np.float32)          # integers below 2^24: exact and distinct
    X = np.ascontiguousarray(np.stack([x, -x], axis=1))
    return X, 2.0 * x.astype(np.float64) + 1.0, (m ** 3 - m) // 3


def end_to_end_keys(n):
    rs = np.random.RandomState(9)
    coef = rs.standard_cauchy(n)
    coef[rs.rand(n) < 0.1] = np.nan
    score = np.round(rs.randn(n), 1)                          # ties
    score[5] = np.nan
    return coef, score


def spearman_table(Xd, V):
    """{(key, gene): scipy.stats.spearmanr(x_g[kept], v_k[kept]).statistic} where it is defined"""
    Xd = np.asarray(Xd, dtype=np.float64)
    V = np.atleast_2d(V)
    kept = np.isfinite(V).all(axis=0)
    out = {}
    for k in range(V.shape[0]):
        for g in range(Xd.shape[1]):
            x, v = Xd[kept, g], V[k, kept]
            if len(x) < 2 or np.isnan(x).any() or np.ptp(x) == 0 or np.ptp(v) == 0:
                continue
            out[(k, g)] = float(scipy.stats.spearmanr(x, v).statistic)
    return out


def assert_matches_scipy(restated, table):
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    rho = rank_corr_statistics(*as_engine(restated))
    assert table
    for (k, g), want in table.items():
        assert abs(rho[k, g] - want) <= RHO_TOL, (k, g, rho[k, g], want)
    dead = np.ones(rho.shape, dtype=bool)
    for k, g in table:
        dead[k, g] = False
    assert np.isnan(rho[dead]).all() and np.isfinite(rho[~dead]).all()
    return rho


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize('form', ['dense-f32', 'dense-f64'])
def test_restatement_is_spearmanr_on_the_core_input(form):
    V = core_keys()
    ref = core_rank_reference(form)
    S, tie_gene, tie_key, m, nan = ref
    codes = core_codes()
    assert m == int((codes >= 0).sum()) - 5 and list(np.flatnonzero(nan)) == [7]
    table = spearman_table(core_input(form), V)
    assert {g for _, g in table} == {1, 3, 4, 6, 8} and {k for k, _ in table} == {0, 1, 2}
    rho = assert_matches_scipy(ref, table)
    assert S[2, 1] == (m ** 3 - m) // 3 and tie_gene[1] == 0.0 and tie_key[2] == 0.0 and tie_key[0] == 0.0 and rho[2, 1] == 1.0
    assert tie_gene[0] == tie_gene[2] == tie_gene[5] == float(m ** 3 - m)    # constant over the kept cells
    assert tie_key[1] > 600.0 ** 3                                           # -0.0 and +0.0 are one group of 600
    assert all(S[k, g] == 0 for k in range(3) for g in (0, 2, 5))


def test_restatement_on_the_other_inputs():
    d = markers_input()
    coef, score = end_to_end_keys(len(d.obs))
    V = np.stack([coef, score])
    ref = restated_rank_corr(d.X, V)
    assert ref[3] == int((np.isfinite(coef) & np.isfinite(score)).sum()) < len(coef)
    assert len(assert_matches_scipy(ref, spearman_table(d.X, V))) == 2
    for q in (1, 16):
        ref = core_rank_reference('dense-f64', q)
        assert ref[0].shape == (q, 9) and ref[3] == core_rank_reference('dense-f64')[3]        # the kept set is key 0's
        rho = assert_matches_scipy(ref, spearman_table(core_input('dense-f64'), core_keys(q)))
        assert rho.shape == (q, 9)
    assert (np.unique(core_keys(16)[3][core_kept()]).size, np.unique(core_keys(16)[6][core_kept()]).size) == (2, 4)


def test_statistics_line_and_the_wide_limbs():
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics, wide_to_float
    vals = [0, 1, -1, 5, -5, 2 ** 53 + 1, -(2 ** 63), 2 ** 63 - 1, 2 ** 63, -(2 ** 63) - 1, 2 ** 64, -(2 ** 64), 3 * 2 ** 90 + 12345,
            -(3 * 2 ** 90) - 12345]
    lo, hi = limbs(np.array([vals], dtype=object))
    got = wide_to_float(lo, hi)[0]
    for v, f in zip(vals, got):
        assert f == float(v) or abs(f - float(v)) <= abs(float(v)) * 2.0 ** -51, v
    assert got[3] == 5.0 and got[4] == -5.0 and got[6] == -2.0 ** 63
    m = WIDE_CELLS
    S = (m ** 3 - m) // 3
    assert S > 2 ** 63 - 1 and S < 2 ** 64                                   # the wide case passes a signed 64-bit sum
    lo, hi = limbs(np.array([[S, -S]], dtype=object))
    assert hi.tolist() == [[0, -1]] and int(lo[0, 0]) == S and int(lo[0, 1]) == 2 ** 64 - S
    rho = rank_corr_statistics(lo, hi, np.zeros(2), np.zeros(1), m, np.zeros(2, dtype=bool))
    np.testing.assert_array_equal(rho, [[1.0, -1.0]])
    # m < 2, a constant key, a constant gene, a flagged gene
    one = np.zeros((1, 2), dtype=np.uint64), np.zeros((1, 2), dtype=np.int64)
    assert np.isnan(rank_corr_statistics(*one, np.zeros(2), np.zeros(1), 1, np.zeros(2, dtype=bool))).all()
    assert np.isnan(rank_corr_statistics(*one, np.zeros(2), np.zeros(1), 0, np.zeros(2, dtype=bool))).all()
    got = rank_corr_statistics(*one, np.array([0.0, 60.0]), np.zeros(1), 4, np.zeros(2, dtype=bool))
    assert got[0, 0] == 0.0 and np.isnan(got[0, 1])
    assert np.isnan(rank_corr_statistics(*one, np.zeros(2), np.array([60.0]), 4, np.zeros(2, dtype=bool))).all()
    got = rank_corr_statistics(*one, np.zeros(2), np.zeros(1), 4, np.array([True, False]))
    assert np.isnan(got[0, 0]) and got[0, 1] == 0.0


# ------------------------------------------------------------------ proofs about the GPU inputs
@pytest.mark.parametrize('form', FORMS)
def test_long_genes_and_keys_span_three_sort_chunks_the_last_one_ragged(form):
    chunks, length = sort_chunks(form)
    assert chunks[1] >= 3 and chunks[2] >= 3 and N_CORE % length != 0
    dense = ranksum_constant('RS_DENSE_CHUNK')                               # a key is a segment of n entries in such chunks
    assert -(-N_CORE // dense) >= 3 and N_CORE % dense != 0


def rank_corr_tiles(form, work_bytes, X=None):
    """ranksum_sorted with the cell as the payload: tiles of whole genes whose entries fit work_bytes / (2 * (key bytes + 4)),
    one gene at least; rankcorr_keys: the columns that fit work_bytes / (2 * (8 + 4)) entries, one at least; of the core input
    in that form, or of the matrix X of that form"""
    X = core_input(form) if X is None else X
    key = 4 if form.endswith('f32') else 8
    budget = work_bytes or ranksum_constant('RS_WORK_BYTES')
    limit = max(1, budget // (2 * (key + 4)))
    length = np.diff(sp.csc_matrix(X).indptr) if sp.issparse(X) else np.full(X.shape[1], X.shape[0])
    seg = np.r_[0, np.cumsum(length)]
    tiles, g0, G = [], 0, len(length)
    while g0 < G:
        g1 = g0 + 1
        while g1 < G and seg[g1 + 1] - seg[g0] <= limit:
            g1 += 1
        tiles.append((g0, g1))
        g0 = g1
    return tiles, limit, length, max(1, max(1, budget // (2 * (8 + 4))) // X.shape[0])


@pytest.mark.parametrize('form', FORMS)
def test_the_small_budget_cuts_at_least_two_tiles_of_genes_and_one_per_key(form):
    assert 'per_entry = 2 * (int64_t)(sizeof(K) + sizeof(P))' in ranksum_source('rank_sort.h')       # ranksum_sorted
    assert 'per_entry = 2 * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t))' in ranksum_source('expr_rankcorr.hip')
    tiles, limit, length, cols = rank_corr_tiles(form, SMALL_WORK_BYTES)
    assert len(tiles) >= 2 and tiles[0][0] == 0 and tiles[-1][1] == 9 and cols == 1
    whole = rank_corr_tiles(form, 0)
    assert len(whole[0]) == 1 and whole[3] >= 16
    assert length[1] > limit                           # a gene that alone exceeds the budget: still one tile


def _runs(col):
    heads = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])
    return {float(col[h]): (int(h), int(e)) for h, e in zip(heads, np.r_[heads[1:], len(col)])}


@pytest.mark.parametrize('form', FORMS)
def test_tie_runs_of_genes_and_keys_meet_the_cuts_of_the_unit(form):
    """k_rc_corr and k_rc_keyrank take a sorted list RS_UNIT at a time.  Gene 4 over THIS call's kept cells: the run of -2.0
    ends exactly on a cut with another value behind it, the run of -1.0 spans two cuts; gene 2 is one run across every cut.
    Key 1: the same two shapes."""
    unit = ranksum_constant('RS_UNIT')
    Vg, Sg = core_values()
    kept = core_kept()
    assert RUN_ON_CUT == unit and RUN_OVER_CUTS > 2 * unit
    use = kept if form.startswith('dense') else kept & Sg[:, 4]
    col = np.sort(Vg[use, 4].astype(np.float32 if form.endswith('f32') else np.float64))
    for runs, n in ((_runs(col), len(col)), (_runs(np.sort(core_keys()[1][kept] + 0.0)), int(kept.sum()))):
        lo, hi = runs[min(runs)]
        assert lo == 0 and hi % unit == 0 and hi < n and hi - lo > 1
        lo, hi = runs[-1.0]
        assert len([c for c in range(unit, n, unit) if lo < c < hi]) >= 2
    assert int(kept.sum()) > 3 * unit and Sg[:, 2].all()
    assert 0.0 in _runs(np.sort(core_keys()[1][kept] + 0.0)) and np.signbit(core_keys()[1][kept]).sum() > 256 + 700


# ------------------------------------------------------------------ the public call
class RankCorrEngine(GeneEngine):
    """GeneEngine (the real residency code, counted uploads) with the device call as numpy."""

    def gene_rank_corr(self, V, work_bytes=0):
        assert self.resident is not None
        return as_engine(restated_rank_corr(self.resident, V))


def test_gene_rank_corr_through_the_public_call():
    import cna_amd as cna
    assert 'gene_rank_corr' in cna.tl.__all__
    d, eng = markers_input(), RankCorrEngine()
    n = len(d.obs)
    d.obs['coef'], d.obs['score'] = end_to_end_keys(n)
    d.var = pd.DataFrame(index=pd.Index(['g%d' % i for i in range(6)]))
    out = cna.tl.gene_rank_corr(d, engine=eng)                                # keys='coef'
    assert isinstance(out, pd.DataFrame) and out.shape == (6, 1) and list(out.columns) == ['coef']
    assert out.index.equals(d.var_names) and (out.dtypes == np.float64).all()
    only = np.isfinite(d.obs['coef'].values)
    assert out.attrs['n_cells'] == int(only.sum())
    Xd = d.X.astype(np.float64)
    for g in range(6):
        want = scipy.stats.spearmanr(Xd[only, g], d.obs['coef'].values[only]).statistic
        assert abs(out['coef'].iloc[g] - want) <= RHO_TOL
    # two keys: the kept set is the intersection, so the first key's column moves
    both = cna.tl.gene_rank_corr(d, ['coef', 'score'], key_added='rho_', engine=eng)
    kept = only & np.isfinite(d.obs['score'].values)
    assert both.shape == (6, 2) and both.attrs['n_cells'] == int(kept.sum()) == int(only.sum()) - 1
    for j, k in enumerate(['coef', 'score']):
        for g in range(6):
            want = scipy.stats.spearmanr(Xd[kept, g], d.obs[k].values[kept]).statistic
            assert abs(both[k].iloc[g] - want) <= RHO_TOL
        np.testing.assert_array_equal(d.var['rho_' + k].values, both[k].values)
    assert not np.array_equal(both['coef'].values, out['coef'].values)
    # invariant to monotone normalisations of the matrix and of a key
    d.layers['log'] = np.ascontiguousarray(np.log1p(d.X - d.X.min()) * 3.0)
    d.obs['cube'] = d.obs['coef'].values ** 3
    logged = cna.tl.gene_rank_corr(d, ['cube', 'score'], layer='log', engine=eng)
    np.testing.assert_array_equal(logged['cube'].values, both['coef'].values)
    np.testing.assert_array_equal(logged['score'].values, both['score'].values)
    assert len(eng.uploads) == 2                                              # X once, the layer once
    bare = _frame(n, X=d.X, coef=d.obs['coef'].values)
    out4 = cna.tl.gene_rank_corr(bare, 'coef', key_added='r_', engine=eng)
    assert isinstance(out4.index, pd.RangeIndex) and list(bare.var.columns) == ['r_coef']
    np.testing.assert_array_equal(out4['coef'].values, out['coef'].values)


def test_nan_rules():
    import cna_amd as cna
    Vg, _ = core_values()
    V = core_keys()
    d = _frame(N_CORE, X=np.ascontiguousarray(Vg), k0=V[0], k1=V[1], k2=V[2], flat=np.where(np.isfinite(V[1]), 4.0, np.nan))
    out = cna.tl.gene_rank_corr(d, ['k0', 'k1', 'k2', 'flat'], engine=RankCorrEngine())
    assert out.shape == (9, 4) and out.attrs['n_cells'] == int(core_kept().sum())
    assert np.isnan(out['flat'].values).all()                                 # a constant key
    for k in ('k0', 'k1', 'k2'):
        col = out[k].values
        assert np.isnan(col[[0, 2, 5, 7]]).all()                              # constant over the kept cells; a kept NaN
        assert np.isfinite(col[[1, 3, 4, 6, 8]]).all()                        # a NaN in a left-out cell does no harm
    assert out['k2'].iloc[1] == 1.0
    # no kept cell, one kept cell
    for keep in (0, 1):
        v = np.full(N_CORE, np.nan)
        v[:keep] = 1.0
        one = cna.tl.gene_rank_corr(_frame(N_CORE, X=np.ascontiguousarray(Vg), v=v), 'v', engine=RankCorrEngine())
        assert one.attrs['n_cells'] == keep and np.isnan(one.values).all()


def test_bad_arguments_and_refusals():
    import cna_amd as cna
    from cna_amd import dist, synth
    d, eng = markers_input(), RankCorrEngine()
    n = len(d.obs)
    d.obs['coef'] = np.arange(n, dtype=float)
    with pytest.raises(KeyError, match='nope'):
        cna.tl.gene_rank_corr(d, ['coef', 'nope'], engine=eng)
    many = _frame(n, X=d.X, **{'k%d' % j: np.arange(n, dtype=float) * (j + 1) for j in range(17)})
    with pytest.raises(ValueError, match='16'):
        cna.tl.gene_rank_corr(many, ['k%d' % j for j in range(17)], engine=eng)
    with pytest.raises(ValueError):
        cna.tl.gene_rank_corr(d, [], engine=eng)
    with pytest.raises(TypeError, match='not numeric'):
        cna.tl.gene_rank_corr(d, 'pop', engine=eng)
    with pytest.raises(ValueError, match='data.X'):
        cna.tl.gene_rank_corr(_frame(n, coef=np.zeros(n)), 'coef', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_rank_corr(d, 'coef', layer='missing', engine=eng)
    with pytest.raises(TypeError):
        cna.tl.gene_rank_corr(_frame(n, X=d.X.astype(np.int32), coef=np.zeros(n)), 'coef', engine=eng)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_rank_corr(d, 'coef', engine=RankCorrEngine(nranks=2))
    data, _ = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    part.obs['coef'] = 1.0
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_rank_corr(part, 'coef', engine=eng)
    assert eng.uploads == []
    assert cna.tl.gene_rank_corr(many, ['k%d' % j for j in range(16)], engine=eng).shape == (6, 16)


def test_entry_is_declared():
    from cna_amd import _ffi
    assert 'cna_gene_rank_corr' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_gene_rank_corr')
    lib = _ffi.load()
    names = [lib.cna_kernel_name(k).decode() for k in range(len(_ffi.KERNELS) + len(_ffi.KERNELS_RANK_CORR))]
    assert names == _ffi.KERNELS + _ffi.KERNELS_RANK_CORR and lib.cna_kernel_name(len(names)) == b'?'
    from cna_amd.engine import Engine
    assert callable(Engine.gene_rank_corr)

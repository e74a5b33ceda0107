"""The inputs of tests/rank_shapes.py on the CPU: that every builder has the property it is named for (tile cuts, chunk
counts, kept against stored entries, the key-count instantiations), that the restatements the GPU tests compare with are
scipy's numbers on these inputs too, and a numpy model of the two pieces of index arithmetic at stake in csrc/rank_sort.h
-- the dense key transposition by RS_TILE x RS_TILE tiles over a tile of genes, and the forward / backward walk in units of
RS_UNIT with its carries -- which equals the direct computation on every new input and stops doing so, on at least one of
them, under each of five deliberate mistakes.  The constants are read from the sources."""
import time

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

import rank_shapes as rs
from test_expr_tiles_host import chunk_length
from test_gene_markers_host import (SMALL_WORK_BYTES, assert_matches_scipy as assert_ranksum_matches_scipy, core_codes,
                                    core_values, mannwhitney_table, ranksum_source, ranksum_tiles, restated_ranksum)
from test_gene_markers_pairs_host import restated_pairs
from test_gene_rank_corr_host import (assert_matches_scipy as assert_rank_corr_matches_scipy, core_kept, restated_rank_corr,
                                      spearman_table)
from test_gene_rank_corr_strata_host import assert_levels_match_scipy, restated_rank_corr_by, strata_kept


# ------------------------------------------------------------------ the builders have the properties they are named for
def test_constants_are_the_sources():
    assert (rs.UNIT, rs.TILE, rs.DENSE_CHUNK, rs.BIG) == (256, 64, 1024, 16)
    assert rs.chunk_floor() == rs.DENSE_CHUNK == chunk_length(0)                 # "build_chunks' least"
    assert rs.AXIS_CELLS == 130 and rs.AXIS_GENES == [64, 65, 130] and rs.AXIS_LEFT == [63, 64, 129]
    # bytes per entry: the level (uint16_t) rides with cna_gene_ranksum_by and _pairs, the cell (uint32_t) with the others
    assert 'per_entry = 2 * (int64_t)(sizeof(K) + sizeof(P))' in ranksum_source('rank_sort.h')
    src = ranksum_source('expr_ranksum.hip')
    assert src.count('ranksum_sorted<T, uint16_t>') == 2 and src.count('ranksum_sorted<T, uint32_t>') == 1
    assert 'ranksum_sorted<T, uint32_t>' in ranksum_source('expr_rankcorr.hip')
    assert 'ranksum_sorted<T, uint32_t>' in ranksum_source('expr_rankperm.hip')
    assert rs.bytes_per_entry('ranksum_by', False) == 12 and rs.bytes_per_entry('rank_corr_wide', True) == 24


@pytest.mark.parametrize('G', rs.AXIS_GENES)
@pytest.mark.parametrize('form', rs.AXIS_FORMS)
def test_gene_axis_case_cuts_the_tiles_it_is_built_for(form, G):
    case = rs.gene_axis_case(form, G)
    f64 = form.endswith('f64')
    n = rs.AXIS_CELLS
    assert case.V.shape == (n, G) and n == 2 * rs.TILE + 2 and -(-n // rs.TILE) == 3
    assert -(-G // rs.TILE) == (1, 2, 3)[rs.AXIS_GENES.index(G)]                  # blocks of genes: blockIdx.y
    for entry in rs.ENTRIES:
        whole, seventy, single = [rs.tiles_of(case, entry, b) for b in rs.axis_budgets(entry, f64)]
        assert whole == [(0, G)]
        assert seventy == ([(0, 70), (70, 130)] if G == 130 else [(0, G)])
        assert single == [(g, g + 1) for g in range(G)]                          # g0 takes every value
    if G == 130:
        # [0, 70): a second 64-block of genes with g1 inside it; [70, 130): g0 = 70, inside a 64-block of the matrix
        assert -(-70 // rs.TILE) == 2 and 70 % rs.TILE != 0 and (130 - 70) < rs.TILE
    # the planted NaNs, and nothing else, are flagged; the left-out cells are left out by code and by key
    ref = rs.reference(case, 'ranksum_by')
    assert list(np.flatnonzero(ref[3])) == sorted(rs.axis_nan_cells(G)) == sorted({g for g in (63, 64, G - 1) if g < G})
    assert all(case.codes[c] >= 0 for c in rs.axis_nan_cells(G).values())
    assert list(np.flatnonzero(case.codes < 0)) == rs.AXIS_LEFT
    assert list(np.flatnonzero(~np.isfinite(case.keys).all(axis=0))) == rs.AXIS_LEFT
    assert list(np.flatnonzero(~np.isfinite(case.wide).all(axis=0))) == rs.AXIS_LEFT
    # ties in every gene, and no two genes alike: two genes that change places change the result
    ok = ~ref[3]
    assert all(len(np.unique(case.V[case.codes >= 0, g])) < 12 for g in np.flatnonzero(ok))
    columns = {tuple(ref[0][:, g]) + (ref[1][g],) for g in np.flatnonzero(ok)}
    assert len(columns) == int(ok.sum())
    # ... and two cells of a gene: every level of a gene holds many of its values, and key 0 tells every cell from the others
    assert all(len(np.unique(case.V[case.codes == l, g])) >= 3 for g in np.flatnonzero(ok) for l in range(rs.LEVELS))
    assert len(np.unique(case.keys[0][case.codes >= 0])) == n - 3


@pytest.mark.parametrize('n', rs.LENGTHS)
def test_length_case_has_the_lists_and_chunks_it_is_built_for(n):
    case = rs.length_case(n, 'csr-f32')
    V, S = case.V, case.S
    assert (case.codes >= 0).all() and np.isfinite(case.keys).all() and np.isfinite(case.wide).all()
    assert list(S.sum(axis=0)) == [n, n, n, n, (n + 1) // 2, 0]
    assert len(np.unique(V[:, 0])) == n and (n < 63 or (V[:, 0].min() < 0 < V[:, 0].max()))
    assert np.ptp(V[:, 1]) == 0
    col = np.sort(V[:, 2])
    assert (col[:n // 2] == -1.0).all() and (col[n // 2:] == 4.0).all()          # the run boundary: position n // 2
    if n >= 12:
        third = [int((V[:, 3] < 0).sum()), int((V[:, 3] == 0).sum()), int((V[:, 3] > 0).sum())]
        assert max(third) - min(third) <= 1 and np.signbit(V[V[:, 3] == 0, 3]).any() and not np.signbit(V[V[:, 3] == 0, 3]).all()
        assert len(np.unique(V[:, 3])) < n // 2
    stored = V[S[:, 4], 4]
    assert (stored != 0).all() and (n < 8 or (stored.min() < 0 < stored.max())) and (n < 2 or (~S[:, 4]).any())
    assert (V[~S] == 0).all()
    # the keys: none tied; runs of 3; key 0 increasing in gene 0, so S = (m^3 - m) / 3 there
    assert len(np.unique(case.keys[0])) == n and (np.argsort(case.keys[0]) == np.argsort(V[:, 0])).all()
    runs = sorted(np.unique(case.keys[1], return_counts=True)[1])
    assert runs == [n % 3] * (n % 3 > 0) + [3] * (n // 3)
    assert list(case.codes[:4]) == [0, 1, 2, 0][:min(n, 4)] and list(case.blocks[:3]) == [0, 1, 0][:min(n, 3)]
    # chunks.  Dense (and every key column): RS_DENSE_CHUNK cells; the stored lists: build_chunks' floor at these sizes
    want = {1023: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 3}
    if n in want:
        assert rs.dense_chunks(n) == want[n]
    assert rs.dense_chunks(n) == -(-n // rs.DENSE_CHUNK) and (n % rs.DENSE_CHUNK == 0) == (n in (1024, 2048))
    for form in ('csr-f32', 'csc-f64'):
        M = rs.upload_of(rs.length_case(n, form))
        assert chunk_length(int(M.nnz)) == rs.chunk_floor()
        lengths = np.diff(sp.csc_matrix(M).indptr)
        assert list(lengths) == [n, n, n, n, (n + 1) // 2, 0]
        assert list(-(-lengths // rs.chunk_floor())) == [rs.dense_chunks(n)] * 4 + [rs.dense_chunks((n + 1) // 2), 0]
    dense = rs.upload_of(rs.length_case(n, 'dense-f32'))
    assert dense.dtype == np.float32 and dense.shape == (n, 6) and np.array_equal(dense.astype(np.float64), V + 0.0)


def test_length_cases_meet_the_unit_the_chunk_and_the_long_run():
    unit = rs.UNIT
    assert {n for n in rs.LENGTHS if n % unit == 0} == {256, 512, 1024, 2048}    # a constant gene ends a full unit
    assert 512 // 2 == unit                                                     # gene 2's run boundary on a unit cut
    for edge in (rs.TILE, unit, 2 * unit, rs.DENSE_CHUNK, 2 * rs.DENSE_CHUNK):
        assert {edge, edge + 1} <= set(rs.LENGTHS) and (edge - 1 in rs.LENGTHS or edge == 2 * rs.DENSE_CHUNK)
    assert {1, 2} <= set(rs.LENGTHS) and max(rs.LENGTHS) == 2049
    # cna_gene_ranksum_pairs hands a tie run of RP_BIG entries to the whole workgroup: gene 3 has shorter and longer ones
    # (the zeros are one group of their own, added at the end)
    def runs(n):
        col = rs.length_case(n, 'csr-f32').V[:, 3]
        return np.unique(col[col != 0], return_counts=True)[1]
    assert runs(65).max() < rs.BIG <= runs(255).min() and 1 < runs(65).min()


@pytest.mark.parametrize('k', rs.KEPT_COUNTS)
def test_kept_case_keeps_k_of_its_stored_entries(k):
    case = rs.kept_case(k)
    kept = case.codes >= 0
    m = int(kept.sum())
    assert m == 560 and m != k and list(np.flatnonzero(~kept)) == list(rs.kept_left())
    assert list(np.flatnonzero(~np.isfinite(case.keys).all(axis=0))) == list(rs.kept_left())
    M = rs.upload_of(case)
    assert M.format == 'csr' and M.dtype == np.float32
    assert list(np.diff(sp.csc_matrix(M).indptr)) == [k + rs.KEPT_LEFT_STORED, rs.KEPT_CELLS, 0]
    assert int((case.S[:, 0] & kept).sum()) == k and int((case.S[:, 0] & ~kept).sum()) == rs.KEPT_LEFT_STORED
    col = np.sort(case.V[case.S[:, 0] & kept, 0])
    if k:
        run = int((col == col[-1]).sum())
        assert run == min(k, 3) and (np.diff(col[:k - run + 1]) > 0).all()       # a tie run that ends at position k - 1
        left = case.V[case.S[:, 0] & ~kept, 0]
        assert (left == col[-1]).sum() == 2 and (left > col[-1]).sum() == 2 and (left < col[0]).sum() == 1
    assert {k for k in rs.KEPT_COUNTS if k and k % rs.UNIT == 0} == {256, 512} and {0, 1, 255, 257} <= set(rs.KEPT_COUNTS)


@pytest.mark.parametrize('n', rs.X_CELLS)
def test_x_case_leaves_out_every_seventh_cell(n):
    x = rs.x_case(n)
    kept = x.xrow >= 0
    assert list(np.flatnonzero(~kept)) == list(range(6, n, 7)) and sorted(x.xrow[kept]) == list(range(x.X.shape[0]))
    assert x.X.shape[1] == rs.X_SAMPLES == 3 and x.Z.shape == (17, 3) and 17 // 16 == 1 and 17 % 16 == 1
    assert np.array_equal(x.X, np.rint(x.X)) and np.array_equal(x.Z, np.rint(x.Z)) and x.Z.any(axis=1).all()
    assert x.case is rs.length_case(n, 'csr-f32')


def width_of(q):
    """with_width of csrc/expr.h: the least of 1, 2, 4, 8, 16 that holds q"""
    return next(w for w in (1, 2, 4, 8, 16) if q <= w or w == 16)


def test_which_key_counts_reach_which_instantiation():
    """k_rc_corr is instantiated per width.  The rank tests so far compare exact integers at 1, 3, 5 and 16 keys: W = 1, 4,
    8 and 16.  Two keys occur there only at m <= 1 kept cells and in the end-to-end frame, which is held to scipy within
    RHO_TOL: W = 2 was never compared integer for integer on a list of any length.  The new cases use q = 2.  The wide and X
    entries always use tables of 16 columns: 17 columns are a full group and a group of one."""
    src = ranksum_source('expr.h')
    for w in (1, 2, 4, 8):
        assert 'if (w <= %d) f(std::integral_constant<int, %d>{});' % (w, w) in src
    assert 'else f(std::integral_constant<int, 16>{});' in src
    assert [width_of(q) for q in (1, 3, 5, 16)] == [1, 4, 8, 16]
    assert width_of(rs.Q) == 2 and rs.Q not in (1, 3, 5, 16)
    assert 'constexpr int RC_MAX_KEYS = 16;' in ranksum_source('rank_corr.h')
    assert 'constexpr int RP_GROUP = RC_MAX_KEYS;' in ranksum_source('expr_rankperm.hip') and rs.Q_WIDE == 16 + 1


# ------------------------------------------------------------------ the restatements against scipy on the new inputs
def _ranksum_against_scipy(case):
    X = rs.typed_values(case)
    ref = restated_ranksum(X, case.codes, rs.LEVELS)
    ok = np.flatnonzero(~ref[3])
    table = mannwhitney_table(X[:, ok], case.codes, rs.LEVELS)
    if table:
        assert_ranksum_matches_scipy(ref[0][:, ok], ref[1][ok], ref[2], ref[3][ok], table)
    # the midranks themselves, doubled and summed per level
    kept = case.codes >= 0
    for g in ok:
        r2 = np.rint(2.0 * scipy.stats.rankdata(X[kept, g].astype(np.float64))).astype(np.int64)
        assert list(ref[0][:, g]) == [int(r2[case.codes[kept] == l].sum()) for l in range(rs.LEVELS)]
    return len(table)


def _pairs_against_scipy(case):
    X = rs.typed_values(case).astype(np.float64)
    u2, tie, n, nan = restated_pairs(X, case.codes, rs.LEVELS, rs.PAIRS)
    checked = 0
    for k, (a, b) in enumerate(rs.PAIRS):
        for g in np.flatnonzero(~nan):
            xa, xb = X[case.codes == a, g], X[case.codes == b, g]
            t = np.unique(np.r_[xa, xb], return_counts=True)[1]
            assert tie[k, g] == float(sum(int(v) ** 3 - int(v) for v in t))
            if len(xa) and len(xb):
                assert u2[k, g] / 2.0 == scipy.stats.mannwhitneyu(xa, xb, use_continuity=False, method='asymptotic').statistic
                checked += 1
            else:
                assert u2[k, g] == 0
    return checked


def _within_against_the_blocks(case):
    """a block alone is cna_gene_ranksum_by on the block's cells: D = rank2 - n_sl (n_s + 1), summed over the blocks"""
    X = rs.typed_values(case)
    d2, num, tiew, live, n, nan = rs.reference(case, 'ranksum_within')
    w_num, w_tie = rs.within_weights_of(case)
    total = np.zeros_like(d2)
    fold_num, fold_tie = np.zeros(d2.shape), np.zeros(d2.shape)
    for s in range(rs.BLOCKS):
        only = np.where(case.blocks == s, case.codes, -1)
        rank2, tie, nl, _ = restated_ranksum(X, only, rs.LEVELS)
        assert list(n[s]) == list(nl)
        D = rank2 - (nl * (int(nl.sum()) + 1))[:, None]
        total += D
        fold_num = fold_num + w_num[s] * D.astype(np.float64)
        fold_tie = fold_tie + w_tie[s][:, None] * tie[None, :]
    ok = ~nan
    np.testing.assert_array_equal(total[:, ok], d2[:, ok])
    np.testing.assert_array_equal(fold_num[:, ok], num[:, ok])
    np.testing.assert_array_equal(fold_tie[:, ok], tiew[:, ok])


def _rank_corr_against_scipy(case):
    X = rs.typed_values(case)
    checked = 0
    for V in (case.keys, case.wide):
        ref = restated_rank_corr(X, V)
        table = spearman_table(X, V)
        if table:
            assert_rank_corr_matches_scipy(ref, table)
        checked += len(table)
    by = restated_rank_corr_by(X, case.keys, case.codes, rs.LEVELS)
    checked += assert_levels_match_scipy(by, X, case.keys, case.codes, rs.LEVELS)
    return checked


@pytest.mark.parametrize('n', rs.LENGTHS)
def test_restatements_are_scipys_numbers_on_every_length(n):
    case = rs.length_case(n, 'csc-f64')
    seen = (_ranksum_against_scipy(case), _pairs_against_scipy(case), _rank_corr_against_scipy(case))
    _within_against_the_blocks(case)
    if n >= 63:
        # genes 0, 2, 3 and 4 vary: every level against the rest, every pair of levels, every key and level
        assert seen[0] == 4 * rs.LEVELS and seen[1] == 6 * len(rs.PAIRS)
        assert seen[2] >= 4 * (rs.Q + rs.Q_WIDE - 1 + rs.LEVELS * rs.Q)
    m = n
    S = restated_rank_corr(case.V, case.keys)[0]
    assert S[0, 0] == (m ** 3 - m) // 3                                          # key 0 increases with gene 0
    ref = rs.reference(case, 'ranksum_by')
    np.testing.assert_array_equal(ref[0][:, 1], ref[2] * (m + 1))               # the constant gene: every cell the midrank
    assert ref[1][1] == ref[1][5] == float(m ** 3 - m) and ref[1][0] == 0.0


@pytest.mark.parametrize('G', rs.AXIS_GENES)
def test_restatements_are_scipys_numbers_on_every_gene_count(G):
    case = rs.gene_axis_case('dense-f64', G)
    live = G - len(rs.axis_nan_cells(G))
    assert _ranksum_against_scipy(case) == live * rs.LEVELS
    assert _pairs_against_scipy(case) == live * len(rs.PAIRS)
    _within_against_the_blocks(case)
    assert _rank_corr_against_scipy(case) >= live * (rs.Q + rs.Q_WIDE + rs.LEVELS * rs.Q) - 3 * G


def test_kept_and_x_cases_are_scipys_numbers_too():
    for k in rs.KEPT_COUNTS:
        case = rs.kept_case(k)
        assert _ranksum_against_scipy(case) == (2 if k > 1 else 1) * rs.LEVELS
        X = rs.typed_values(case)
        assert_rank_corr_matches_scipy(restated_rank_corr(X, case.keys), spearman_table(X, case.keys))
        if k == 0:
            ref, corr = rs.reference(case, 'ranksum_by'), rs.reference(case, 'rank_corr')
            np.testing.assert_array_equal(ref[0][:, 0], ref[0][:, 2])           # no kept entry: a gene without entries
            assert ref[1][0] == ref[1][2] and (corr[0][:, 0] == 0).all() and corr[1][0] == corr[1][2]
    for n in rs.X_CELLS:
        x = rs.x_case(n)
        V = rs.x_columns_of(x)
        keep = x.xrow >= 0
        assert np.array_equal(V[:, keep].T, x.X[x.xrow[keep]] @ x.Z.T) and np.isnan(V[:, ~keep]).all()
        table = spearman_table(x.case.V, V)
        if n > 1:
            assert_rank_corr_matches_scipy(restated_rank_corr(x.case.V, V), table)


def test_every_tie_term_is_an_integer_a_double_holds():
    for case in [rs.length_case(max(rs.LENGTHS), 'csc-f64'), rs.gene_axis_case('dense-f64', 130), rs.kept_case(512)]:
        assert rs.largest_tie_term(case) < 2 ** 53


def test_the_time_of_the_references_is_printed():
    """printed for profiles/rank_shapes_parity.txt: the restatements of the six entries on the largest case of each kind"""
    line = []
    for name, case in (('axis G=130 dense-f64', rs.gene_axis_case('dense-f64', 130)),
                       ('n=2049 csc-f64', rs.length_case(2049, 'csc-f64')), ('k=512', rs.kept_case(512)),
                       ('x n=1025', rs.x_case(1025).case)):
        t0 = time.perf_counter()
        for entry in rs.ENTRIES:
            rs.reference(case, entry)
        line.append('%s %.3f s' % (name, time.perf_counter() - t0))
    print('CPU time of the six restatements per id: ' + ', '.join(line))


# ------------------------------------------------------------------ the numpy model of the index arithmetic
LEFT = np.inf                       # the model's all-ones key: what an entry of a left-out cell gets
DENSE_MISTAKES = ['g < g1 dropped', 'gene0 taken without g0']
WALK_MISTAKES = ['the forward carry dropped at a unit cut', 'the backward walk started at k / RS_UNIT * RS_UNIT',
                 'the backward carry taken from a ragged unit']


def model_dense_keys(X, kept, g0, g1, mistake=None):
    """k_rs_keys_dense on the tile [g0, g1) of the dense X [n, G], block by block as the kernel goes: every workgroup loads
    RS_TILE cells x RS_TILE genes into tk[cell][gene] (the all-ones key for what the guards leave out) and stores them
    transposed at gene * n + cell - base with the cell as the payload.  Returns {index: (key, cell)} of everything written."""
    n, G = X.shape
    T = rs.TILE
    flat = X.ravel()
    base = g0 * n
    guard = mistake != 'g < g1 dropped'
    out = {}
    for by in range(-(-(g1 - g0) // T)):
        gene0 = (0 if mistake == 'gene0 taken without g0' else g0) + by * T
        for bx in range(-(-n // T)):
            i = bx * T + np.arange(T)
            g = gene0 + np.arange(T)
            tl = np.where(i < n, np.where(kept[np.minimum(i, n - 1)], i, -1), -1)
            load = (i < n)[:, None] & ((g < g1)[None, :] | (not guard)) & (tl >= 0)[:, None]
            at = i[:, None] * G + g[None, :]
            load &= at < flat.size                                               # (beyond the matrix: whatever lies there)
            tk = np.full((T, T), LEFT)
            tk[load] = flat[at[load]]
            store = ((g < g1) | (not guard))[:, None] & (i < n)[None, :]           # [gene r][cell tx]
            to = g[:, None] * n + i[None, :] - base
            keys, cells = tk.T, np.broadcast_to(tl[None, :], (T, T))
            for a, k, c in zip(to[store], keys[store], cells[store]):
                out[int(a)] = (float(k), int(c))
    return out


def direct_dense_keys(X, kept, g0, g1):
    n = X.shape[0]
    out = {}
    for g in range(g0, g1):
        for i in range(n):
            out[(g - g0) * n + i] = (float(X[i, g]) if kept[i] else LEFT, i if kept[i] else -1)
    return out


def _same_writes(a, b):
    if a.keys() != b.keys():
        return False
    ka, kb = np.array([a[j] for j in sorted(a)]), np.array([b[j] for j in sorted(b)])
    return np.array_equal(ka, kb, equal_nan=True)


def model_walk(key, k, mistake=None):
    """rs_walk_forward and rs_walk_backward over the k kept entries in front of the sorted `key`, RS_UNIT at a time with the
    kernels' carries.  Returns (s, e, units): the tie run [s, e) of every kept entry and the units the two walks took."""
    U = rs.UNIT
    t = np.arange(U)
    s, e = np.full(k, -9, dtype=np.int64), np.full(k, -9, dtype=np.int64)
    units = 0
    carry = 0
    for u0 in range(0, k, U):
        p = u0 + t
        valid = p < k
        pv = p[valid]
        head = np.zeros(U, dtype=bool)
        head[valid] = (pv == 0) | (key[np.maximum(pv - 1, 0)] != key[pv])
        v = np.where(head, p, -1)
        if not head[0] and mistake != 'the forward carry dropped at a unit cut':
            v[0] = carry
        scan = np.maximum.accumulate(v)
        carry = scan[U - 1]
        s[pv] = scan[valid]
        units += 1
    none = -0x7fffffffffffffff
    carry = 0
    if mistake == 'the backward walk started at k / RS_UNIT * RS_UNIT':
        u0 = k // U * U
    else:
        u0 = (k - 1) // U * U if k > 0 else -1
    while u0 >= 0:
        p = u0 + t
        valid = p < k
        pv = p[valid]
        tail = np.zeros(U, dtype=bool)
        tail[valid] = (pv == k - 1) | (key[np.minimum(pv + 1, len(key) - 1)] != key[pv])
        v = np.where(tail, -(p + 1), none)
        carries = valid[U - 1] or mistake == 'the backward carry taken from a ragged unit'
        if not tail[U - 1] and carries:
            v[U - 1] = carry
        scan = np.maximum.accumulate(v[::-1])[::-1]
        carry = scan[0]
        e[pv] = -scan[valid]
        units += 1
        u0 -= U
    return s, e, units


def direct_walk(key, k):
    _, first, inverse, counts = np.unique(key[:k], return_index=True, return_inverse=True, return_counts=True)
    s = first[inverse].astype(np.int64).reshape(k)
    return s, s + counts[inverse].reshape(k), 2 * -(-k // rs.UNIT)


def sorted_list(values, kept):
    """(key, k): the entries of one list as the sort leaves them, the kept ones by value (-0.0 is +0.0) in front of the
    left-out ones with the all-ones key"""
    front = np.sort(values[kept] + 0.0)
    return np.r_[front, np.full(int((~kept).sum()), LEFT)], len(front)


def lists_of(V, S, kept, splits=()):
    """every list a walk sees: per gene without a kept NaN the dense list (every cell) and the stored one, whole and inside
    every level of each split (cna_gene_rank_corr_by's levels, cna_gene_ranksum_within's blocks)"""
    for g in range(V.shape[1]):
        if np.isnan(V[kept, g]).any():
            continue
        for entries in ((np.ones(len(kept), dtype=bool), S[:, g]) if S is not None else (np.ones(len(kept), dtype=bool),)):
            yield sorted_list(V[entries, g], kept[entries])
            for codes in splits:
                for l in range(int(codes.max()) + 1):
                    inside = entries & kept & (codes == l)
                    yield sorted_list(V[inside, g], np.ones(int(inside.sum()), dtype=bool))


def new_walk_lists():
    for n in rs.LENGTHS:
        c = rs.length_case(n, 'csr-f32')
        yield from lists_of(c.V, c.S, c.codes >= 0, (c.codes, c.blocks))
    for G in rs.AXIS_GENES:
        c = rs.gene_axis_case('dense-f64', G)
        yield from lists_of(c.V, None, c.codes >= 0, (c.codes, c.blocks))
    for k in rs.KEPT_COUNTS:
        c = rs.kept_case(k)
        yield from lists_of(c.V, c.S, c.codes >= 0)
    for n in rs.X_CELLS:
        x = rs.x_case(n)
        yield from lists_of(x.case.V, x.case.S, x.xrow >= 0)


def old_walk_lists():
    V, S = core_values()
    yield from lists_of(V, S, core_codes() >= 0)
    yield from lists_of(V, S, core_kept(), (strata_kept(),))


def new_dense_tiles():
    """(X, kept, g0, g1) of every tile of genes the dense cases are cut into under their budgets"""
    for G in rs.AXIS_GENES:
        c = rs.gene_axis_case('dense-f64', G)
        seventy = rs.tiles_of(c, 'ranksum_by', rs.axis_budgets('ranksum_by', True)[1])
        for tiles in ([(0, G)], seventy, [(g, g + 1) for g in range(G)]):
            for g0, g1 in tiles:
                yield c.V, c.codes >= 0, g0, g1
    for n in rs.LENGTHS:
        c = rs.length_case(n, 'dense-f32')
        for g0, g1 in [(0, 6)] + [(g, g + 1) for g in range(6)]:
            yield c.V, c.codes >= 0, g0, g1


def old_dense_tiles():
    V, _ = core_values()
    for form in ('dense-f32', 'dense-f64'):
        for budget in (0, SMALL_WORK_BYTES):
            for g0, g1 in ranksum_tiles(form, budget)[0]:
                yield V, core_codes() >= 0, g0, g1


def _dense_differs(tiles, mistake):
    return any(not _same_writes(model_dense_keys(X, kept, g0, g1, mistake), direct_dense_keys(X, kept, g0, g1))
               for X, kept, g0, g1 in tiles)


def _walk_differs(lists, mistake):
    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    return any(not same(model_walk(key, k, mistake), direct_walk(key, k)) for key, k in lists)


def test_the_model_is_the_direct_computation_on_every_new_input():
    tiles = list(new_dense_tiles())
    assert len(tiles) > 2 * 130 and not _dense_differs(tiles, None)
    lists = list(new_walk_lists())
    assert len(lists) > 1000 and {k for _, k in lists} >= {0, 1, 2, 63, 64, 65, 255, 256, 257, 512, 1024, 2048, 2049}
    assert any(len(key) > k for key, k in lists) and not _walk_differs(lists, None)
    assert not _dense_differs(old_dense_tiles(), None) and not _walk_differs(old_walk_lists(), None)


def test_each_deliberate_mistake_changes_the_model_on_a_new_input():
    """Five mistakes in the index arithmetic, each of which the new inputs tell from the right code.  One of them, the backward
    walk begun at k / RS_UNIT * RS_UNIT, cannot change s or e: when RS_UNIT divides k it walks one unit of no entries first,
    whose carry no thread takes.  What it changes is the number of units walked, which is why the model returns that count
    beside s and e; the lists of 256, 512, 1024 and 2048 entries show it, and so does a list without entries.  Likewise a
    dropped `g < g1` leaves the tile's own entries as they are: what the model shows is the writes outside them.  The printed
    line says which of the five the old 3001-cell input shows as well (profiles/rank_shapes_parity.txt)."""
    new_tiles, old_tiles = list(new_dense_tiles()), list(old_dense_tiles())
    new_lists, old_lists = list(new_walk_lists()), list(old_walk_lists())
    caught = {m: (_dense_differs(new_tiles, m), _dense_differs(old_tiles, m)) for m in DENSE_MISTAKES}
    caught.update({m: (_walk_differs(new_lists, m), _walk_differs(old_lists, m)) for m in WALK_MISTAKES})
    print('deliberate mistakes, caught by the new inputs / by the old core input: '
          + '; '.join('%s: %s / %s' % (m, 'yes' if new else 'NO', 'yes' if old else 'no') for m, (new, old) in caught.items()))
    assert len(caught) == 5
    for m, (new, _) in caught.items():
        assert new, m
    # where the new inputs are the only ones: a second 64-block of genes, and a list that is a whole number of units
    V130 = rs.gene_axis_case('dense-f64', 130)
    blocks_y = lambda tiles: max(-(-(g1 - g0) // rs.TILE) for _, _, g0, g1 in tiles)
    assert blocks_y(old_tiles) == 1 and blocks_y(new_tiles) == 3 and V130.V.shape[1] == 130
    assert not any(k and k % rs.UNIT == 0 for _, k in old_lists) and any(k and k % rs.UNIT == 0 for _, k in new_lists)

"""CPU checks of tests/walk_exact.py, the inputs and references of tests/test_gpu_walk_exact.py: the integer reference
against fractions.Fraction, the sequential restatement against the project's oracle (scipy's A.dot), every condition the
patterns were designed to meet, and the restated launcher table against the width list.  Nothing here skips: a case that
does not meet its condition fails."""
import fractions

import numpy as np
import pytest

import walk_exact as wx
from oracle import cna_oracle as orc


def _oracle_states(A, pat, nsteps, s0=None, w=1):
    cs = orc.column_sums(A, w, 'f64')
    s = wx.onehot(pat).astype(bool) if s0 is None else s0
    out = []
    for i in range(nsteps):
        s = orc.diffusion_step(A, s, cs, w, first_onehot=(s0 is None and i == 0), mode='f64')
        out.append(s)
    return out


def _small_pattern(n, N, seed, with_zero):
    rs = np.random.RandomState(seed)
    rows = []
    for r in range(n):
        d = int(rs.choice([0, 1, 2, 5, 9, n - 1]))
        c = rs.choice(n - 1, d, replace=False)
        rows.append(c + (c >= r))
    deg = np.array([len(x) for x in rows])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    zero = np.zeros(len(indices), dtype=bool)
    if with_zero:
        zero[rs.choice(len(indices), 4, replace=False)] = True
    return wx.Pattern(n, N, indptr, indices, wx._codes(rs, n, N), zero, {})


@pytest.mark.parametrize('n,N,w,with_zero,dense_m', [(37, 5, 1, False, 0), (40, 40, 1, True, 0), (23, 7, 0.25, True, 0),
                                                     (31, 1, 1, False, 3), (40, 3, 0.25, True, 4)])
def test_integer_reference_equals_fraction_arithmetic(n, N, w, with_zero, dense_m):
    """exact_walk against the definition evaluated in rationals: colsums = A.sum(axis=0) + w, s <- A.(s / colsums) +
    w s / colsums.  Every float64 entry must be the rational itself."""
    F = fractions.Fraction
    pat = _small_pattern(n, N, 11 * n + N, with_zero)
    A = wx.exact_matrix(pat, np.float64, w)
    s0 = wx.dense_input(pat, 'exact', dense_m) if dense_m else None
    got = wx.exact_walk(pat, 3, s0=s0, self_weight=w)
    dense = A.toarray()
    assert (dense[np.repeat(np.arange(n), np.diff(pat.indptr))[pat.zero], pat.indices[pat.zero]] == 0).all()
    Af = [[F(v) for v in row] for row in dense]
    cs = [sum(Af[i][j] for i in range(n)) + F(w) for j in range(n)]
    s = [[F(int(v)) for v in row] for row in (wx.onehot(pat) if s0 is None else s0)]
    m = len(s[0])
    for step in range(3):
        T = [[s[i][c] / cs[i] for c in range(m)] for i in range(n)]
        s = [[sum(Af[i][j] * T[j][c] for j in range(n) if Af[i][j]) + F(w) * T[i][c] for c in range(m)] for i in range(n)]
        for i in range(n):
            for c in range(m):
                assert F(float(got.s[step][i, c])) == s[i][c], (step, i, c)
    # ... and it is what the float64 flows give on these inputs, in either order of the roundings
    start = wx.onehot(pat) if s0 is None else s0
    for a, b, c in zip(got.s, wx.sequential_walk(A, start, 3, w), _oracle_states(A, pat, 3, s0, w)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


CASES = ([('ladder', N, n) for N, n in wx.WIDTH_CASES] + [('ladder', N, N + 331) for N in wx.PLACEMENT_N]
         + [('balanced', N, wx.width_cells(N)) for N in wx.STATE32_N]
         + [('pair_limit', N, wx.pair_limit_cells(N)) for N in wx.PAIR_LIMIT_N]
         + [('collisions', N, N + 140) for N in wx.PAIR_LIMIT_N])


def _pattern(kind, N, n):
    if kind in ('ladder', 'balanced'):
        return wx.ladder(n, N, N, balanced=kind == 'balanced')
    return (wx.pair_limit if kind == 'pair_limit' else wx.collisions)(n, N, N)


WIDTHS_FOUND = {}


def _widths(kind, N, n, ew=None):
    if (kind, N, n) not in WIDTHS_FOUND:
        ew = ew or wx.exact_walk(_pattern(kind, N, n), wx.NSTEPS)
        WIDTHS_FOUND[kind, N, n] = (max(ew.t_bits), max(ew.s_bits), max(ew.num_bits))
    return WIDTHS_FOUND[kind, N, n]


@pytest.mark.parametrize('kind,N,n', CASES, ids=['%s-N%d-n%d' % c for c in CASES])
def test_references_agree_and_the_pattern_holds_what_it_was_designed_to(kind, N, n):
    """On every pattern the GPU module walks, at every size it walks it: the sequential restatement equals
    oracle.diffusion_step(mode='f64') for float32 and float64 weights, and on the exact family the integer reference equals
    both; every sample owns a cell; every column sum of the exact family is a power of two; numerators stay below 2^53
    (exact_walk asserts it); and the pattern's own design conditions hold."""
    pat = _pattern(kind, N, n)
    n, N = pat.n, pat.N
    assert pat.indices.dtype == np.int32 and len(pat.codes) == n
    assert (np.bincount(pat.codes, minlength=N) >= 1).all() and pat.codes.max() == N - 1
    deg = np.diff(pat.indptr)
    rows = np.repeat(np.arange(n), deg)
    assert (pat.indices != rows).all() and 0 <= pat.indices.min() and pat.indices.max() < n
    key = rows.astype(np.int64) * n + pat.indices
    assert len(np.unique(key)) == len(key)                               # distinct neighbours
    ew = wx.exact_walk(pat, wx.NSTEPS)
    _widths(kind, N, n, ew)
    assert max(ew.t_bits + ew.s_bits) <= 53
    for fam in wx.FAMILIES:
        A = wx.family_matrix(pat, fam)
        assert A.dtype == (np.float64 if fam == 'f64' else np.float32) and A.indices.dtype == np.int32
        assert (A.data[pat.zero] == 0).all() and (A.data[~pat.zero] > 0).all()
        np.testing.assert_array_equal(wx.column_sums(A, 1), orc.column_sums(A, 1, 'f64'))
        ref = wx.reference_states(pat, fam, A)
        for a, b in zip(ref, _oracle_states(A, pat, wx.NSTEPS)):
            np.testing.assert_array_equal(a, b)
        if fam == 'exact':
            cs = orc.column_sums(A, 1, 'f64')
            assert (np.frexp(cs)[0] == 0.5).all()                        # powers of two
            for a, b in zip(ref, wx.sequential_walk(A, wx.onehot(pat), wx.NSTEPS)):
                np.testing.assert_array_equal(a, b)
        else:
            # 40 binades: the weights really make the order of the additions matter
            lg = np.log2(A.data[~pat.zero].astype(np.float64))
            assert lg.max() - lg.min() > 35
    first = ew.s[0]
    nz = (first != 0).sum(axis=1)
    if kind in ('ladder', 'balanced'):
        assert set(deg.tolist()) == set(wx.LADDER)                        # every degree of the ladder, at every size
        assert set(wx.DESIGNED_ROW_PAIRS) <= set(zip(deg[0::2].tolist(), deg[1::2].tolist()))
        if kind == 'balanced':
            # the four-byte state: what a walk stores between its steps fits a float32 significand
            assert max(ew.t_bits) <= 24, ew.t_bits
            cnt = np.bincount(pat.indices, minlength=n)
            assert cnt.max() <= 64                                        # no hub column
        elif N >= wx.SPARSE_MIN_N:
            assert (nz > wx.SP_CAP).any() and (nz <= wx.SP_CAP).any()      # overflowed rows and compressed ones
    elif kind == 'pair_limit':
        targets, gathered = pat.info['targets'], pat.info['gathered']
        for r, count, dense in targets:
            assert nz[r] == count and dense == (count > wx.SP_CAP)
        assert sorted(set(c for _, c, _ in targets)) == [62, 63, 64, 65]
        own_in = {}
        for r, count, dense in targets:
            nb = pat.indices[pat.indptr[r]:pat.indptr[r + 1]]
            live = ~pat.zero[pat.indptr[r]:pat.indptr[r + 1]]
            own_in.setdefault(count, set()).add(bool((pat.codes[nb[live]] == pat.codes[r]).any()))
            if not live.all():                       # 65 distinct samples, one behind a stored 0.0: still 64 pairs
                assert len(set(pat.codes[nb].tolist())) == 65 and count == 64 and live.sum() == 64
        assert all(v == {True, False} for v in own_in.values()), own_in
        assert sum(1 for r, c, d in targets if pat.zero[pat.indptr[r]:pat.indptr[r + 1]].any()) == 3
        # layouts: first chunk only, last chunk only (where a chunk is full), spread over every chunk
        chunks = [set((np.flatnonzero(first[r]) // 64).tolist()) for r, c, d in targets]
        nchunk = (N + 63) // 64
        assert any(ch == {0} for ch in chunks) and any(ch == set(range(nchunk)) for ch in chunks)
        assert any(np.array_equal(np.flatnonzero(first[r]), np.arange(N - c, N)) for r, c, d in targets)
        if N % 64 == 0:                              # (else the last chunk is too short to hold 62 samples)
            assert any(ch == {nchunk - 1} for ch in chunks)
        # how the second step meets an overflowed row: inside a batch of five, in the ragged tail, in a load of 64
        # edges with no other overflowed row, next to a load of 64 with none
        where = set()
        for r, count, dense in targets:
            for g, pos in gathered[r]:
                assert pat.indices[pat.indptr[g] + pos] == r
                d = int(deg[g])
                if not dense:
                    assert d == 12
                    where.add(('pairs', 'batch' if pos < 10 else 'tail'))
                    continue
                nb = pat.indices[pat.indptr[g]:pat.indptr[g + 1]]
                over = nz[nb] > wx.SP_CAP
                assert nz[g] <= wx.SP_CAP                                 # the gatherer itself stays compressed
                if d == 12:
                    where.add('batch' if pos < 10 else 'tail')
                else:
                    assert d == 130 and 64 <= pos < 128 and over.sum() == 1 and not over[:64].any()
                    where.add('load of 64, alone')
                    where.add('after a load with none')
        assert where >= {'batch', 'tail', 'load of 64, alone', 'after a load with none', ('pairs', 'batch'),
                         ('pairs', 'tail')}, where
        assert any(nz[r] == wx.SP_CAP for r, c, d in targets)
    else:
        r64, r130 = pat.info['rows']
        assert deg[r64] == 64 and deg[r130] == 130
        for r in (r64, r130):
            nb = pat.indices[pat.indptr[r]:pat.indptr[r + 1]]
            assert (pat.codes[nb] == pat.info['sample']).all()
            assert nz[r] == (1 if pat.codes[r] == pat.info['sample'] else 2)


def test_row_counts_and_significand_widths():
    """The row counts of the widths test cover every residue mod 8 and the small ends n = N, N + 1, N + 3; the widest
    significands of the exact family, per kind of pattern, are printed (profiles/walk_exact_parity.txt records them) and
    bounded: 24 bits for what the four-byte walk stores, 53 for everything else."""
    assert {n % 8 for N, n in wx.WIDTH_CASES} == set(range(8))
    assert {(N, n - N) for N, n in wx.WIDTH_CASES} >= {(320, 0), (509, 1), (1021, 3)}
    for which in ('ladder', 'balanced', 'pair_limit', 'collisions'):
        w = np.array([_widths(*c) for c in CASES if c[0] == which])
        t_bits, s_bits, num_bits = w.max(axis=0)
        assert t_bits <= (24 if which == 'balanced' else 53) and s_bits <= 53 and num_bits <= 53
        print('largest widths (%s, %d cases): stored state %d bits, state %d bits, numerator over the common denominator '
              '%d bits'
              % (which, len(w), t_bits, s_bits, num_bits))


def test_width_list_reaches_every_instantiation_of_the_launcher():
    """diffuse.hip:launch_step_q restated (walk_exact.dispatch): the widths of the GPU module reach every instantiation of
    every step kernel, and every width reaches the one it was put on the list for."""
    first, sparse, later, dense2, st32 = set(), set(), set(), set(), set()
    for N, n in wx.WIDTH_CASES:
        first.add(wx.dispatch(N, n, 1))
        s2 = wx.dispatch(N, n, 2)
        assert (s2[0] == 'k_nam_step_sparse') == (N >= 96)
        (sparse if N >= 96 else later).add(s2)
        later.add(wx.dispatch(N, n, 3))
        dense2.add(wx.dispatch(N, n, 2, sparse_min_n=0))
    for N in wx.PLACEMENT_N:
        later.add(wx.dispatch(N, N + 331, 3))
        later.add(wx.dispatch(N, N + 331, 3, step_wide=True))
    for N in wx.STATE32_N:
        st32.add(wx.dispatch(N, wx.width_cells(N), 3, in32=True))
        st32.add(wx.dispatch(N, wx.width_cells(N), 3, in32=True, step32_wide=True))
    assert first == {(k, q) for k in ('k_nam_first', 'k_nam_first2') for q in (1, 2, 3, 4, 6, 8, 12, 16)}
    assert sparse == {('k_nam_step_sparse', q) for q in (1, 2, 3, 4, 6, 8)}
    steps = {('k_nam_step', 1, 8), ('k_nam_step', 2, 10), ('k_nam_step', 3, 8), ('k_nam_step', 4, 8), ('k_nam_step', 6, 4),
             ('k_nam_step', 8, 4)}
    assert later == steps | {('k_nam_step_pair',)}
    assert dense2 == later                                   # CNA_SPARSE_MIN_N=0: the same kernels on the second step
    assert st32 == {('k_nam_step32h',), ('k_nam_step32', 1, 8), ('k_nam_step32', 2, 8), ('k_nam_step32', 3, 4),
                    ('k_nam_step32', 4, 4)}
    # the by-product's own instantiation of 129 ... 256 columns (test_selection_as_a_by_product_of_the_last_walk_step)
    assert wx.dispatch(200, 20011, 3, select=True) == ('k_nam_step', 2, 8)
    # each width, and what it is on the list for: the two sides and the last column of every boundary of the table
    meant = {1: (1, None, 'pair'), 3: (1, None, 'pair'), 61: (1, None, 'pair'), 64: (1, None, 'pair'),
             65: (2, None, 1), 95: (2, None, 1), 96: (2, 1, 1), 125: (2, 1, 1), 128: (2, 1, 1),
             129: (3, 2, 2), 189: (3, 2, 2), 192: (3, 2, 2), 193: (4, 2, 2), 253: (4, 2, 2), 256: (4, 2, 2),
             257: (6, 3, 3), 320: (6, 3, 3), 321: (6, 3, 3), 384: (6, 3, 3), 385: (8, 4, 4), 509: (8, 4, 4), 512: (8, 4, 4),
             513: (12, 6, 6), 765: (12, 6, 6), 768: (12, 6, 6), 769: (16, 8, 8), 1021: (16, 8, 8), 1024: (16, 8, 8)}
    assert sorted(meant) == sorted(wx.WIDTHS)
    for N in wx.WIDTHS:
        n = wx.width_cells(N)
        nq, sp_q, step_q = meant[N]
        assert wx.dispatch(N, n, 1)[1] == nq
        s2, s3 = wx.dispatch(N, n, 2), wx.dispatch(N, n, 3)
        assert s2 == (('k_nam_step_sparse', sp_q) if sp_q else s3)
        if step_q == 'pair':
            assert s3 == ('k_nam_step_pair',)
        else:
            assert s3[:2] == ('k_nam_step', step_q) and s3[2] == {1: 8, 2: 10, 3: 8, 4: 8, 6: 4, 8: 4}[step_q]
    print('instantiations reached:', sorted(first), sorted(sparse), sorted(later), sorted(st32))


@pytest.mark.parametrize('w', [1, 0.25])
def test_dense_diffusion_references(w):
    """The inputs of the dense diffusion test: the integer reference and oracle.diffuse(mode='f64') agree on the exact
    family for both self weights, column sums are powers of two with either, and the sequential restatement is the oracle
    on the other two."""
    pat = wx.ladder(wx.DENSE_CELLS, 1, 3)
    for m in (1, 65):
        for fam in wx.FAMILIES:
            A = wx.family_matrix(pat, fam, w)
            s0 = wx.dense_input(pat, fam, m)
            ref = wx.reference_states(pat, fam, A, 2, s0=s0, self_weight=w)
            np.testing.assert_array_equal(ref[-1], orc.diffuse(A, s0.astype(np.float64), 2, self_weight=w, mode='f64'))
            if fam == 'exact':
                assert (np.frexp(orc.column_sums(A, w, 'f64'))[0] == 0.5).all()


def test_first_diff_names_row_column_and_degree():
    a = np.zeros((4, 3))
    b = a.copy()
    assert wx.first_diff(a, b) is None
    b[2, 1] = 1.0
    msg = wx.first_diff(a, b, degrees=[5, 6, 7, 8], what='step 2')
    assert 'row 2 (degree 7), column 1' in msg and msg.startswith('step 2')
